// forge3d_amd/csrc/f3d_smoke.hip -- smoke volume ray-marcher on gfx950 (BASELINE.json config 5).
//
// Reference: SmokeVolume::raymarch_rgba / raymarch_projection_rgba / march_ray_rgba / sun_transmittance,
// src/smoke/render.rs:7-330 with sampling.rs and types.rs -- single-threaded CPU Rust, six separate f32 fields,
// every field sampled at every step.  Here: one lane per pixel, 8x8 pixel tiles per wave (neighbouring rays walk
// neighbouring voxels), and the six fields re-packed into two records per voxel so that a trilinear tap is
// 8 x dwordx4 (+ 8 x dwordx2 only where there is smoke):
//     A = (density, soot, age, temperature)   everything the extinction and the self-shadow march need
//     B = (humidity, emission)                colour / glow only, read when density > 1e-5 like the reference's use
// Results are bit-identical to oracle/smoke_oracle.c (same operation order, no contraction, exp_det).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <mutex>
#include <new>
#include <vector>

#include "f3d_setup.h"
#include "f3d_devmem.h"
#include "f3d_div_known.h"

using namespace f3d;

namespace {

struct SmokeSettingsDev {
    float density_scale, extinction, scattering, absorption, phase_g;
    uint32_t max_steps, self_shadow, shadow_steps;
    float jitter_strength, exposure, soot_absorption, fire_glow;
    V3 thin, dense;
};

struct SmokeParams {
    const float4 *rec_a;  // density, soot, age, temperature
    const float2 *rec_b;  // humidity, emission
    uint32_t nx, ny, nz;
    V3 origin, voxel, bmin, bmax;
    V3 voxel_rcp;        // RN(1 / voxel) per axis, for div_known()
    uint32_t known_div;  // != 0: every voxel size is a divisor div_known() is exact for (the host checks; see there)
    const uint8_t *occupied;  // per low corner (or block of low corners, kOccShift): does a tap there touch any density != 0?
    uint32_t ocx, ocy;        // blocks along x, y
    const uint32_t *bounds;   // of the marked entries of `occupied`: lowest x, y, z, then ~highest x, y, z (k_smoke_bounds)
    uint32_t clip;            // 0: the box is not used (a voxel size that is not a positive finite number)
    uint32_t frame_index, width, height, mode;  // mode 0 perspective, 1 projection
    V3 eye, forward, right, camera_up, sun, view;
    float tan_half_fov, aspect, diagonal, step, shadow_step;
    SmokeSettingsDev st;
    uint8_t *out;
};

// Empty-space map (round 5).  Most of a ray's steps, and most of a self-shadow march, cross voxels that hold NO smoke at all:
// density exactly 0 at all eight corners of the tap.  Such a step changes nothing -- the interpolated density is 0, the
// reference's own `density > 1e-5` test skips it (render.rs:226-228), and a self-shadow step adds +0 to the optical depth
// (render.rs:308-322) -- but it still cost eight 16-byte gathers from L2, which is what this kernel is bound by (VALU issue
// 0.33, lane use 0.93: profiles/r04_config_rooflines.json).  k_smoke_pack therefore also marks, per tap LOW corner (a byte
// a voxel: 786 KB for the 96 x 64 x 128 domain, L2-resident; -DF3D_SMOKE_OCC_SHIFT=2 is the first form, a byte per 4 x 4 x 4
// block of low corners, which also skipped nothing in the 2-3 voxel shell around the plume), whether a tap with its low
// corner there touches a voxel whose density is not +-0; a step whose mark is clear is taken without its loads.  Exact, not a
// threshold: only taps that are zero at every corner are skipped, so images stay bit-identical to the oracle's (tests/test_smoke.py).
#ifndef F3D_SMOKE_OCC_SHIFT
#define F3D_SMOKE_OCC_SHIFT 0
#endif
constexpr uint32_t kOccShift = F3D_SMOKE_OCC_SHIFT;
struct PackParams {
    const float *density, *temperature, *soot, *humidity, *emission, *age;
    float4 *rec_a;
    float2 *rec_b;
    uint64_t n;
    uint8_t *occupied;
    uint32_t nx, ny, nz, ocx, ocy;
};

__global__ void k_smoke_pack(const PackParams P) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n) return;
    const float d = P.density[i];
    P.rec_a[i] = float4{d, P.soot[i], P.age[i], P.temperature[i]};
    P.rec_b[i] = float2{P.humidity[i], P.emission[i]};
    if (d != 0.0f) {  // (also true for a NaN: never skipped)
        // voxel (x, y, z) is a corner of the taps whose low corner is (x - 1 .. x, y - 1 .. y, z - 1 .. z)
        const uint32_t x = (uint32_t)(i % P.nx), y = (uint32_t)((i / P.nx) % P.ny), z = (uint32_t)(i / ((uint64_t)P.nx * P.ny));
        const uint32_t bx1 = x >> kOccShift, by1 = y >> kOccShift, bz1 = z >> kOccShift;
        const uint32_t bx0 = (x ? x - 1u : 0u) >> kOccShift, by0 = (y ? y - 1u : 0u) >> kOccShift, bz0 = (z ? z - 1u : 0u) >> kOccShift;
        for (uint32_t bz = bz0; bz <= bz1; bz++)
            for (uint32_t by = by0; by <= by1; by++)
                for (uint32_t bx = bx0; bx <= bx1; bx++) P.occupied[(bz * P.ocy + by) * P.ocx + bx] = 1u;  // (every writer stores the same byte)
    }
}

// The box of the marked entries of the empty-space map, for smoke_box(): a workgroup per z slice of the map leaves the slice's
// bounds (x, y; the upper ones as their complements, so that "nothing marked" is all ones), a single wave folds the slices.
// (A first form folded with atomicMin from every wave: 28 us of same-address atomics for a 7 us pack kernel.)
__global__ __launch_bounds__(256) void k_smoke_bounds(const uint8_t *occupied, uint32_t ocx, uint32_t ocy, uint4 *slices) {
    __shared__ uint4 part[4];
    const uint32_t z = blockIdx.x, per_slice = ocx * ocy;
    uint32_t lx = 0xFFFFFFFFu, ly = 0xFFFFFFFFu, hx = 0xFFFFFFFFu, hy = 0xFFFFFFFFu;  // minima; hx, hy of the complements
    for (uint32_t i = threadIdx.x; i < per_slice; i += 256u)
        if (occupied[(size_t)z * per_slice + i] != 0u) {
            const uint32_t x = i % ocx, y = i / ocx;
            lx = min(lx, x);
            ly = min(ly, y);
            hx = min(hx, ~x);
            hy = min(hy, ~y);
        }
    for (int o = 32; o > 0; o >>= 1) {
        lx = min(lx, (uint32_t)__shfl_xor((int)lx, o, 64));
        ly = min(ly, (uint32_t)__shfl_xor((int)ly, o, 64));
        hx = min(hx, (uint32_t)__shfl_xor((int)hx, o, 64));
        hy = min(hy, (uint32_t)__shfl_xor((int)hy, o, 64));
    }
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = uint4{lx, ly, hx, hy};
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint4 r = part[0];
        for (int w = 1; w < 4; w++) r = uint4{min(r.x, part[w].x), min(r.y, part[w].y), min(r.z, part[w].z), min(r.w, part[w].w)};
        slices[z] = r;
    }
}
__global__ __launch_bounds__(64) void k_smoke_bounds_fold(const uint4 *slices, uint32_t n_slices, uint32_t *bounds) {
    uint32_t v[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};  // lx ly lz ~hx ~hy ~hz
    for (uint32_t z = threadIdx.x; z < n_slices; z += 64u) {
        const uint4 s = slices[z];
        if (s.x == 0xFFFFFFFFu) continue;
        v[0] = min(v[0], s.x);
        v[1] = min(v[1], s.y);
        v[2] = min(v[2], z);
        v[3] = min(v[3], s.z);
        v[4] = min(v[4], s.w);
        v[5] = min(v[5], ~z);
    }
    for (int o = 32; o > 0; o >>= 1)
        for (int k = 0; k < 6; k++) v[k] = min(v[k], (uint32_t)__shfl_xor((int)v[k], o, 64));
    if (threadIdx.x == 0u)
        for (int k = 0; k < 6; k++) bounds[k] = v[k];
}

__device__ __forceinline__ float lerp_ref(float a, float b, float t) { return a + (b - a) * t; }  // sampling.rs:88-90
__device__ __forceinline__ V3 vadd(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 vscale(V3 a, float s) { return V3{a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ float vdot(V3 a, V3 b) { return (a.x * b.x) + (a.y * b.y) + (a.z * b.z); }  // glam order

// trilinear tap set of grid_coord_from_world + sample_scalar (types.rs:375-381, sampling.rs:1-34)
struct Tap {
    uint32_t i000, dx, dy, dz;  // linear index of the low corner, strides to the high ones (0 at the border)
    uint32_t block;             // of the empty-space map (see k_smoke_pack)
    float fx, fy, fz;
};
__device__ __forceinline__ Tap make_tap(const SmokeParams &P, V3 pos) {
    const float ax = pos.x - P.origin.x, ay = pos.y - P.origin.y, az = pos.z - P.origin.z;
    float gx, gy, gz;
#if !defined(F3D_SMOKE_PLAIN_DIV)
    if (P.known_div != 0u && f_max(f_max(f_abs(ax), f_abs(ay)), f_abs(az)) < kDivKnownMax) {
        gx = div_known(ax, P.voxel.x, P.voxel_rcp.x) - 0.5f;
        gy = div_known(ay, P.voxel.y, P.voxel_rcp.y) - 0.5f;
        gz = div_known(az, P.voxel.z, P.voxel_rcp.z) - 0.5f;
    } else
#endif
    {
        gx = ax / P.voxel.x - 0.5f;
        gy = ay / P.voxel.y - 0.5f;
        gz = az / P.voxel.z - 0.5f;
    }
    const float x = f_clamp(gx, 0.0f, (float)(P.nx - 1u)), y = f_clamp(gy, 0.0f, (float)(P.ny - 1u)),
                z = f_clamp(gz, 0.0f, (float)(P.nz - 1u));
    const uint32_t x0 = (uint32_t)f_floor(x), y0 = (uint32_t)f_floor(y), z0 = (uint32_t)f_floor(z);
    Tap t;
    t.i000 = (z0 * P.ny + y0) * P.nx + x0;
    t.block = ((z0 >> kOccShift) * P.ocy + (y0 >> kOccShift)) * P.ocx + (x0 >> kOccShift);
    t.dx = x0 + 1u < P.nx ? 1u : 0u;
    t.dy = y0 + 1u < P.ny ? P.nx : 0u;
    t.dz = z0 + 1u < P.nz ? P.nx * P.ny : 0u;
    t.fx = x - (float)x0;
    t.fy = y - (float)y0;
    t.fz = z - (float)z0;
    return t;
}
__device__ __forceinline__ float tri(const Tap &t, float c000, float c100, float c010, float c110, float c001, float c101,
                                     float c011, float c111) {
    const float c00 = lerp_ref(c000, c100, t.fx), c10 = lerp_ref(c010, c110, t.fx);
    const float c01 = lerp_ref(c001, c101, t.fx), c11 = lerp_ref(c011, c111, t.fx);
    return lerp_ref(lerp_ref(c00, c10, t.fy), lerp_ref(c01, c11, t.fy), t.fz);
}
#define F3D_TRI(buf, member)                                                                                    \
    tri(t, buf[t.i000].member, buf[t.i000 + t.dx].member, buf[t.i000 + t.dy].member, buf[t.i000 + t.dx + t.dy].member, \
        buf[t.i000 + t.dz].member, buf[t.i000 + t.dx + t.dz].member, buf[t.i000 + t.dy + t.dz].member,               \
        buf[t.i000 + t.dx + t.dy + t.dz].member)

__device__ __forceinline__ float smoothstep_ref(float e0, float e1, float x) {  // render_smoothstep, render.rs:405-408
    const float t = f_clamp((x - e0) / f_max(e1 - e0, 1.0e-6f), 0.0f, 1.0f);
    return t * t * (3.0f - 2.0f * t);
}
// ... with edges that are literals at every call: the width and its reciprocal fold to constants (f3d_div_known.h; the static
// assertions of `SmoothEdges` keep the two pairs of edges in use inside what it is exact for)
template <int WHICH>
struct SmoothEdges;
template <>
struct SmoothEdges<0> {  // the age ramp, render.rs:227 / :312
    static constexpr float e0 = 1.6f, e1 = 17.0f;
};
template <>
struct SmoothEdges<1> {  // the density gate, render.rs:228 / :313
    static constexpr float e0 = 0.045f, e1 = 0.34f;
};
template <int WHICH>
__device__ __forceinline__ float smoothstep_known(float x) {
    constexpr float e0 = SmoothEdges<WHICH>::e0, e1 = SmoothEdges<WHICH>::e1;
    constexpr float d = (e1 - e0) > 1.0e-6f ? (e1 - e0) : 1.0e-6f, r = 1.0f / d;
    static_assert((__builtin_bit_cast(uint32_t, d) & 0x7FFFFFu) != 0x7FFFFFu && d > 0x1p-40f && d < 0x1p40f, "div_known needs another divisor");
    const float a = x - e0;
#if !defined(F3D_SMOKE_PLAIN_DIV)
    const float q = f_abs(a) < kDivKnownMax ? div_known(a, d, r) : a / d;
#else
    const float q = a / d;
#endif
    const float t = f_clamp(q, 0.0f, 1.0f);
    return t * t * (3.0f - 2.0f * t);
}

// ray_box_intersection, render.rs:363-392 (f32::min / max ignore a NaN operand, like fminf / fmaxf)
__device__ __forceinline__ bool ray_box(V3 o, V3 d, V3 mn, V3 mx, float &near_t, float &far_t) {
    const float inf = __builtin_inff();
    const float ix = f_abs(d.x) > 1.0e-12f ? 1.0f / d.x : inf, iy = f_abs(d.y) > 1.0e-12f ? 1.0f / d.y : inf,
                iz = f_abs(d.z) > 1.0e-12f ? 1.0f / d.z : inf;
    const float ax = (mn.x - o.x) * ix, bx = (mx.x - o.x) * ix, ay = (mn.y - o.y) * iy, by = (mx.y - o.y) * iy,
                az = (mn.z - o.z) * iz, bz = (mx.z - o.z) * iz;
    near_t = f_max(f_max(f_min(ax, bx), f_min(ay, by)), f_min(az, bz));
    far_t = f_min(f_min(f_max(ax, bx), f_max(ay, by)), f_max(az, bz));
    return far_t >= f_max(near_t, 0.0f);
}

// The smoke's bounding box (round 5).  Most of the steps the empty-space map answers are nowhere near the plume: a camera ray
// crosses the whole domain, the plume fills a part of it, and even a skipped step costs the tap's three IEEE divisions, its
// clamps and the map's byte -- 60 vector instructions, on ~150 steps of each of two million rays: the larger part of the
// 336 M vector instructions of a launch (profiles/r05_C5_rocprofv3_summary.txt).  k_smoke_bounds reduces the map to the
// box of its marked low corners; a ray (and a self-shadow march) is clipped against that box, widened by a voxel and by a
// bound on what float rounding can move a position or a slab parameter, and the steps outside the clipped interval are
// taken without looking anything up: they are steps the map would have answered "empty" -- same image, bit for bit.
struct SmokeBox {
    V3 lo, hi;     // world space; -inf / +inf where the box touches a clamped end of the grid (or is not used)
    V3 inv_sun;    // 1 / P.sun, to a few ulp (the margins below are thousands of ulp)
    uint32_t any;  // 0: no voxel holds smoke
};
__device__ __forceinline__ V3 inv3(V3 d) { return V3{__frcp_rn(d.x), __frcp_rn(d.y), __frcp_rn(d.z)}; }
__device__ __forceinline__ SmokeBox smoke_box(const SmokeParams &P) {
    SmokeBox b;
    const uint32_t l[3] = {P.bounds[0], P.bounds[1], P.bounds[2]}, h[3] = {~P.bounds[3], ~P.bounds[4], ~P.bounds[5]};
    const uint32_t n[3] = {P.nx, P.ny, P.nz};
    const float o[3] = {P.origin.x, P.origin.y, P.origin.z}, v[3] = {P.voxel.x, P.voxel.y, P.voxel.z};
    float lo[3], hi[3];
    b.any = l[0] != 0xFFFFFFFFu ? 1u : 0u;
    for (int a = 0; a < 3; a++) {
        // low corners c0 .. c1 (map blocks -> corners); a tap has low corner c for positions in [c + 0.5, c + 1.5) voxels from
        // the origin, the first and the last corner also for everything the clamp folds onto them
        const uint32_t c0 = l[a] << kOccShift, c1 = ((h[a] + 1u) << kOccShift) - 1u;
        lo[a] = (c0 == 0u || P.clip == 0u) ? -__builtin_inff() : o[a] + ((float)c0 - 0.5f) * v[a];
        hi[a] = (c1 + 1u >= n[a] || P.clip == 0u) ? __builtin_inff() : o[a] + ((float)c1 + 2.5f) * v[a];
    }
    b.lo = V3{lo[0], lo[1], lo[2]};
    b.hi = V3{hi[0], hi[1], hi[2]};
    b.inv_sun = inv3(P.sun);
    return b;
}
// [ta, tb]: outside it no point o + d t (as the march evaluates it in float) has a tap with a marked low corner.  Any NaN
// leaves a bound that no comparison trips.
__device__ __forceinline__ void smoke_clip(const SmokeBox &b, V3 o, V3 d, V3 inv_d, float t_max, float &ta, float &tb) {
    const float err = 1.0e-5f * ((f_abs(o.x) + f_abs(o.y) + f_abs(o.z)) + f_abs(t_max) * (f_abs(d.x) + f_abs(d.y) + f_abs(d.z)));
    const float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z}, ii[3] = {inv_d.x, inv_d.y, inv_d.z};
    const float lo[3] = {b.lo.x, b.lo.y, b.lo.z}, hi[3] = {b.hi.x, b.hi.y, b.hi.z};
    ta = -__builtin_inff();
    tb = __builtin_inff();
    for (int a = 0; a < 3; a++) {
        const float l = lo[a] - err, h = hi[a] + err;
        if (f_abs(dd[a]) > 1.0e-12f) {
            const float p = (l - oo[a]) * ii[a], q = (h - oo[a]) * ii[a];
            ta = f_max(ta, f_min(p, q));
            tb = f_min(tb, f_max(p, q));
        } else if (oo[a] < l || oo[a] > h) {
            ta = __builtin_inff();
            tb = -__builtin_inff();
        }
    }
    ta -= 1.0e-5f * f_abs(ta);
    tb += 1.0e-5f * f_abs(tb);
    if (b.any == 0u) {
        ta = __builtin_inff();
        tb = -__builtin_inff();
    }
}

// sun_transmittance, render.rs:290-330
__device__ float sun_transmittance(const SmokeParams &P, const SmokeBox &box, V3 start) {
    float t0, t1;
    if (!ray_box(vadd(start, vscale(P.sun, P.shadow_step)), P.sun, P.bmin, P.bmax, t0, t1)) return 1.0f;
    t0 = f_max(t0, 0.0f);
    float od = 0.0f;
    uint32_t i = 0u, i_end = P.st.shadow_steps;
#if !defined(F3D_SMOKE_NO_SKIP) && !defined(F3D_SMOKE_NO_CLIP)
    {   // steps whose position start + sun (shadow_step + tt) is outside the smoke's box add +-0: the loop starts and ends at the box
        float ua, ub;
        smoke_clip(box, start, P.sun, box.inv_sun, P.shadow_step * (float)(P.st.shadow_steps + 2u) + t0, ua, ub);
        const float base = P.shadow_step + t0;  // position parameter of step i: base + (i + 0.5) shadow_step
        const float per = __frcp_rn(P.shadow_step);
        const float first = f_floor((ua - base) * per - 0.5f) - 2.0f, last = __builtin_ceilf((ub - base) * per - 0.5f) + 2.0f;
        i = (uint32_t)f_min(f_max(first, 0.0f), (float)i_end);
        i_end = (uint32_t)f_min(f_max(last, 0.0f), (float)i_end);
    }
#endif
    bool in_smoke = false;  // the step before this one had smoke under it: this one is not asked about, its gathers go out at once
    for (; i < i_end; i++) {
        const float tt = t0 + ((float)i + 0.5f) * P.shadow_step;
        if (tt > t1) break;
        const Tap t = make_tap(P, vadd(start, vscale(P.sun, P.shadow_step + tt)));
#if !defined(F3D_SMOKE_NO_SKIP)  // A/B + test-of-the-tests switch
        // density +-0 at all eight corners: the step adds +-0 to od (and od > 8 was tested when it last grew).  The map only
        // ever saves work -- a step that is evaluated although its corners are all zero adds the same +-0 -- so inside the
        // plume, where the answer is almost always "occupied", the byte's round trip is left out
        if (!in_smoke && P.occupied[t.block] == 0u) continue;
#endif
        const float density = F3D_TRI(P.rec_a, x), soot = F3D_TRI(P.rec_a, y), age = f_max(F3D_TRI(P.rec_a, z), 0.0f);
#if !defined(F3D_SMOKE_ALWAYS_ASK)
        in_smoke = density != 0.0f;
#endif
        const float age_t = smoothstep_known<0>(age);
        const float gate = 0.50f + 0.50f * smoothstep_known<1>(density);
        od += density * P.st.density_scale * (1.0f - 0.58f * age_t) * gate * P.st.extinction *
              (1.0f + soot * P.st.soot_absorption) * P.shadow_step;
        if (od > 8.0f) break;
    }
    // f32::clamp hands a NaN back (render.rs:315) where fminf / fmaxf would drop it: a march that crossed a NaN density leaves
    // the pixel's colour NaN, which to_u8 writes as 0, and its alpha untouched (tests/test_smoke.py, the non-finite case)
    const float tr = exp_det(-od);
    return tr != tr ? tr : f_clamp(tr, 0.0f, 1.0f);
}

__device__ __forceinline__ V3 mix3(V3 a, V3 b, float t) {
    return V3{lerp_ref(a.x, b.x, t), lerp_ref(a.y, b.y, t), lerp_ref(a.z, b.z, t)};
}
__device__ __forceinline__ uint8_t to_u8(float v) { return (uint8_t)(f_clamp(v, 0.0f, 1.0f) * 255.0f + 0.5f); }

// The in-scattered + emitted radiance of a step (march_ray, render.rs:237-283; smoke_color :343-361)
__device__ __forceinline__ V3 smoke_source(const SmokeParams &P, V3 p, float s_density, float s_soot, float s_age, float s_temperature, float s_humidity,
                                           float s_emission, float sigma_t, float light, float phase) {
        // smoke_color, render.rs:343-361
        const float body = f_clamp(s_density * 1.45f + s_soot * 1.35f, 0.0f, 1.0f);
        V3 col = mix3(P.st.thin, P.st.dense, body);
        col = mix3(col, V3{0.36f, 0.39f, 0.43f}, f_clamp(s_age / 9.0f, 0.0f, 1.0f) * 0.42f);
        const float milk = f_clamp(s_humidity, 0.0f, 1.0f) * (0.18f + 0.42f * body);
        col = mix3(col, V3{0.93f, 0.92f, 0.84f}, f_clamp(milk, 0.0f, 0.38f));
        const float freshness = f_clamp(1.0f - s_age / 17.0f, 0.0f, 1.0f);
        col = mix3(col, V3{0.95f, 0.62f, 0.28f}, f_clamp(s_temperature * 0.12f * freshness, 0.0f, 1.0f) * 0.07f);

        const float albedo = f_clamp(P.st.scattering / (P.st.scattering + P.st.absorption + s_soot * 0.55f + 1.0e-5f), 0.02f, 0.98f);
        const float sigma_s = sigma_t * albedo;
        const V3 sun_rad = vscale(V3{1.0f, 0.96f, 0.84f}, 11.5f);
        const V3 sky = vscale(vscale(V3{0.52f, 0.60f, 0.72f}, 0.36f + 0.26f * f_clamp(1.0f - light, 0.0f, 1.0f)),
                              f_clamp(1.0f - s_soot * 0.32f, 0.50f, 1.0f));
        const V3 bounce = vscale(vscale(V3{0.58f, 0.54f, 0.48f}, 0.070f), f_clamp(1.0f - p.y / f_max(P.bmax.y, 1.0f), 0.0f, 1.0f));
        const float powder = f_clamp(1.0f - exp_det(-sigma_t * P.step * 2.2f), 0.0f, 1.0f);
        const float pw = powder * 0.055f * f_sqrt(light);
        const V3 cs = vscale(col, sigma_s);
        const V3 multiple = cs * vadd(vadd(sky, bounce), V3{pw, pw, pw});
        const V3 direct = vscale(vscale(cs * sun_rad, phase), light);
        const float fresh_heat = s_temperature * freshness * freshness;
        const V3 emission = vscale(V3{1.0f, 0.30f, 0.055f}, f_clamp((fresh_heat * 0.10f + s_emission * 1.18f) * P.st.fire_glow, 0.0f, 5.0f));
        return vadd(vadd(direct, multiple), emission);
}
// ... and the pixel a finished ray leaves (render.rs:284-288)
__device__ __forceinline__ uchar4 smoke_pixel(const SmokeParams &P, V3 rgb, float transmittance) {
    const float alpha = f_clamp(1.0f - transmittance, 0.0f, 1.0f);
    const V3 straight = alpha > 1.0e-5f ? V3{rgb.x / alpha, rgb.y / alpha, rgb.z / alpha} : rgb;
    const V3 e = vscale(straight, P.st.exposure);
    return uchar4{to_u8(e.x / (1.0f + e.x)), to_u8(e.y / (1.0f + e.y)), to_u8(e.z / (1.0f + e.z)), to_u8(alpha)};
}

// ---- the self-shadow marches taken out of the rays' loops (round 5) ---------------------------------------------------------
// Per wave clocks of the one-kernel form on the configs[4] frame (tools/experiments/smoke_tile_clock.py): the launch takes
// 1.21 ms and ONE wave of it runs for 1.17 ms -- the 8 x 8 tile through the thickest part of the plume, ~100 steps in smoke,
// each with a self-shadow march of 20 steps, every step ~200 vector instructions issued by a wave that is alone on its SIMD
// once the light tiles have drained -- while the waves of the whole launch add up to 0.76 ms per SIMD at one wave a SIMD.
// The launch is as long as its longest ray.  But the reference's loop only needs the self-shadow march's result for the
// radiance it adds (render.rs:237-283): the ray's own course -- which steps meet smoke, the transmittance, where it ends --
// does not depend on it.  So the marches are independent of each other and of their rays, and the frame is taken in three
// launches:
//   k_smoke_rays<kCollect>  a lane per pixel walks its ray without the self-shadow marches and without the radiance, and
//                   writes every step that meets smoke -- its position, the six interpolated fields, its extinction and its
//                   transmittance -- to a slot of a chunked list: the lane's k-th such step of tile T goes to chunk
//                   chunk_of[T][k / 16], row k % 16, column = lane (chunks handed out from a cursor as the tile's wave needs
//                   them; the 64 lanes of a row are the tile's pixels at the same ordinal: neighbouring voxels, as in the
//                   one-kernel form);
//   k_smoke_light   a lane per slot, 64 slots a wave, waves striding over the chunks handed out: the self-shadow march from
//                   that position (sun_transmittance, unchanged) -- 20 steps deep instead of 100 x 20, and as many waves as
//                   the chip can hold;
//   k_smoke_shade   a lane per pixel adds up the radiance of its listed steps in their order (smoke_source, unchanged): no
//                   ray to walk any more, and loads whose addresses do not depend on what was loaded before.
// Each value is computed by the same instructions from the same operands as in the one-kernel form, so the image is the
// oracle's bit for bit (tests/test_smoke.py runs all forms).  When the list's space runs out, the tile is flagged and
// k_smoke_shade walks its rays in the one-kernel form.
enum : uint32_t { kWhole = 0u, kCollect = 1u };
constexpr uint32_t kChunkRows = 16u, kChunkSlots = kChunkRows * 64u, kNoChunk = 0xFFFFFFFFu, kUnset = 0xFFFFFFFEu;
// Sizing of the deferred list (f3d_smoke_render): 4 in-volume steps per pixel, at most 1 GiB.  Round 5 took 16 a pixel and a cap
// of 5.6 GB -- 1.7 GB at 1080p, held per stream for the life of the process (round-5 advice).  Measured on BASELINE configs[4]
// (1080p, 96 x 64 x 128 plume, frame 160): 3 373 chunks used of the 8 100 this gives (f3d_smoke_seq_stats; 432 MB).  A tile whose
// steps do not fit is walked in the one-kernel form by k_smoke_shade: slower, same pixels.
constexpr size_t kListStepsPerPixel = 4u, kListCapMb = 1024u;
constexpr const char *kShadowCursorTag = "smoke.render.shadow.cursor";  // the list's fill count (read by f3d_smoke_seq_stats)
struct Deferred {
    float4 *where;       // per slot: the step's position, and its extinction sigma_t
    float4 *fields;      // per slot: density, soot, age, temperature as interpolated there
    float4 *more;        // per slot: humidity, emission, the step's transmittance, -
    float *light;        // per slot: the self-shadow march's result (k_smoke_light)
    uint32_t *spilled;   // [tile]: != 0 when the list had no room for all of the tile's steps
    uint32_t *chunk_of;  // [tile][chunks_per_tile]
    uint2 *owner;        // [chunk]: (tile, which 16 ordinals of it)
    uint32_t *count;     // [pixel]: steps of the pixel's ray that met smoke
    uint32_t *cursor;    // chunks handed out
    uint32_t chunks_per_tile, capacity;  // capacity in chunks
};

// The slot of the lane's k-th smoke step, reserving the chunk if the tile has none for it yet (kNoChunk: no room left).
__device__ __forceinline__ uint32_t deferred_slot(const Deferred &D, volatile uint32_t *wave_chunks, uint32_t tile, uint32_t k) {
    const uint32_t c = k / kChunkRows, lane = threadIdx.x & 63u;
    uint32_t id = wave_chunks[c];
    while (id == kUnset) {  // one pass per chunk that lanes of the wave wait for
        if (lane == (uint32_t)__builtin_ctzll(__ballot(1))) {
            uint32_t fresh = atomicAdd(D.cursor, 1u);
            if (fresh >= D.capacity) fresh = kNoChunk;
            else D.owner[fresh] = uint2{tile, c};
            D.chunk_of[(size_t)tile * D.chunks_per_tile + c] = fresh;
            wave_chunks[c] = fresh;
        }
        id = wave_chunks[c];
    }
    return id == kNoChunk ? kNoChunk : id * kChunkSlots + (k % kChunkRows) * 64u + lane;
}

// march_ray_rgba, render.rs:192-288
template <uint32_t MODE>
__device__ uchar4 march_ray(const SmokeParams &P, const SmokeBox &box, V3 origin, V3 dir, float t0, float t1, uint32_t seed,
                            const Deferred &D, volatile uint32_t *wave_chunks, uint32_t tile, uint32_t &smoke_steps) {
    uint32_t v = seed;  // hash01, sampling.rs:96-103
    v ^= v >> 16;
    v *= 0x7FEB352Du;
    v ^= v >> 15;
    v *= 0x846CA68Bu;
    v ^= v >> 16;
    const float jitter = ((float)v / 4294967296.0f - 0.5f) * P.st.jitter_strength * P.step;
    float t = f_max(t0 + jitter, 0.0f), transmittance = 1.0f;
    V3 rgb = V3{0.0f, 0.0f, 0.0f};
    const float cos_theta = f_clamp(vdot(dir, P.sun), -1.0f, 1.0f);
    const float g2 = P.st.phase_g * P.st.phase_g;  // henyey_greenstein, render.rs:394-398 (powf(d, 1.5) = d sqrt(d))
    const float denom = f_max(1.0f + g2 - 2.0f * P.st.phase_g * cos_theta, 1.0e-4f);
    const float phase = (1.0f - g2) / (4.0f * kPi * (denom * f_sqrt(denom)));
    uint32_t steps = 0u, k = 0u;
    bool in_smoke = false;
#if !defined(F3D_SMOKE_NO_SKIP) && !defined(F3D_SMOKE_NO_CLIP)
    float ta, tb;
    smoke_clip(box, origin, dir, inv3(dir), t1, ta, tb);
    for (; t < t1 && steps < P.st.max_steps && t < ta; steps++, t += P.step) {}  // in front of the smoke's box: the reference's loop, nothing to look up
#endif
    for (; t < t1 && steps < P.st.max_steps && transmittance > 0.01f; steps++, t += P.step) {
#if !defined(F3D_SMOKE_NO_SKIP) && !defined(F3D_SMOKE_NO_CLIP)
        if (t > tb) break;  // behind it (P.step > 0): every step still to come would be skipped
#endif
        const V3 p = vadd(origin, vscale(dir, t));
        const Tap tp = make_tap(P, p);
#if !defined(F3D_SMOKE_NO_SKIP)
        // density +-0 at all eight corners: the reference's `density > 1e-5` test skips the step (asked only when the step
        // before had no smoke: see sun_transmittance)
        if (!in_smoke && P.occupied[tp.block] == 0u) continue;
#endif
        const Tap &t_ = tp;
#define t t_
        const float s_density = F3D_TRI(P.rec_a, x), s_soot = F3D_TRI(P.rec_a, y), s_age = f_max(F3D_TRI(P.rec_a, z), 0.0f);
#undef t
#if !defined(F3D_SMOKE_ALWAYS_ASK)
        in_smoke = s_density != 0.0f;
#endif
        const float age_t = smoothstep_known<0>(s_age);
        const float gate = 0.50f + 0.50f * smoothstep_known<1>(s_density);
        const float density = f_max(s_density * P.st.density_scale * (1.0f - 0.58f * age_t) * gate, 0.0f);
        if (!(density > 1.0e-5f)) continue;
        const float sigma_t = density * P.st.extinction * (1.0f + s_soot * P.st.soot_absorption * 0.85f);
        const float seg_tr = f_clamp(exp_det(-sigma_t * P.step), 0.0f, 1.0f);
#define t t_
        const float s_temperature = F3D_TRI(P.rec_a, w), s_humidity = F3D_TRI(P.rec_b, x), s_emission = F3D_TRI(P.rec_b, y);
#undef t
        if (MODE == kCollect) {
            const uint32_t slot = deferred_slot(D, wave_chunks, tile, k);
            if (slot != kNoChunk) {
                D.where[slot] = float4{p.x, p.y, p.z, sigma_t};
                D.fields[slot] = float4{s_density, s_soot, s_age, s_temperature};
                D.more[slot] = float4{s_humidity, s_emission, seg_tr, 0.0f};
            } else {
                wave_chunks[D.chunks_per_tile] = 1u;  // the tile's "spilled" flag
            }
        } else {
            const float seg_w = sigma_t > 1.0e-6f ? (1.0f - seg_tr) / sigma_t : P.step;
            const float light = P.st.self_shadow ? sun_transmittance(P, box, p) : 1.0f;
            const V3 source = smoke_source(P, p, s_density, s_soot, s_age, s_temperature, s_humidity, s_emission, sigma_t, light, phase);
            rgb = vadd(rgb, vscale(vscale(source, seg_w), transmittance));
        }
        k++;
        transmittance *= seg_tr;
    }
    smoke_steps = k;
    return smoke_pixel(P, rgb, transmittance);
}

// the ray of pixel (x, y) and the seed of its jitter
__device__ __forceinline__ void pixel_ray(const SmokeParams &P, uint32_t x, uint32_t y, V3 &origin, V3 &dir, uint32_t &seed) {
    seed = x * 73856093u + y * 19349663u + P.frame_index;
    if (P.mode == 0u) {  // raymarch_rgba, render.rs:69-75
        const float px = (((float)x + 0.5f) / (float)P.width * 2.0f - 1.0f) * P.aspect * P.tan_half_fov;
        const float py = (1.0f - ((float)y + 0.5f) / (float)P.height * 2.0f) * P.tan_half_fov;
        const V3 d = vadd(vadd(P.forward, vscale(P.right, px)), vscale(P.camera_up, py));
        dir = vscale(d, 1.0f / f_sqrt(vdot(d, d)));
        origin = P.eye;
    } else {  // raymarch_projection_rgba, render.rs:140-160
        const float fz = ((float)y + 0.5f) / (float)P.height, fx = ((float)x + 0.5f) / (float)P.width;
        const V3 plane = V3{lerp_ref(P.bmin.x, P.bmax.x, fx), (P.bmin.y + P.bmax.y) * 0.5f, lerp_ref(P.bmin.z, P.bmax.z, fz)};
        dir = P.view;
        origin = V3{plane.x - dir.x * P.diagonal, plane.y - dir.y * P.diagonal, plane.z - dir.z * P.diagonal};
        seed += 0x9e3779b9u;
    }
}

// One lane per pixel, 8 x 8 pixels a wave.  MODE kWhole: the whole ray with its self-shadow marches (the form of rounds 3-4: runs
// when a render has no self-shadowing, and as F3D_SMOKE_MARCH=single); kCollect: see "taken out of the rays' loops".
__device__ __forceinline__ bool tile_pixel(const SmokeParams &P, uint32_t tile, uint32_t lane, uint32_t &x, uint32_t &y) {
    const uint32_t tiles_x = (P.width + 7u) / 8u;
    x = (tile % tiles_x) * 8u + (lane & 7u);
    y = (tile / tiles_x) * 8u + (lane >> 3);
    return x < P.width && y < P.height;
}
template <uint32_t MODE>
__device__ __forceinline__ void walk_pixel(const SmokeParams &P, const Deferred &D, volatile uint32_t *wave_chunks, uint32_t x, uint32_t y) {
    V3 origin, dir;
    uint32_t seed;
    pixel_ray(P, x, y, origin, dir, seed);
    uchar4 px4 = uchar4{0, 0, 0, 0};
    float t0, t1;
    const SmokeBox box = smoke_box(P);
#if defined(F3D_SMOKE_TILE_CLOCK)  // diagnostic build (tools/experiments/smoke_tile_clock.py): when each wave ran, in the first pixels of its tile
    const uint64_t clock0 = wall_clock64();
#endif
    uint32_t smoke_steps = 0u;
    if (ray_box(origin, dir, P.bmin, P.bmax, t0, t1))
        px4 = march_ray<MODE>(P, box, origin, dir, f_max(t0, 0.0f), t1, seed, D, wave_chunks, blockIdx.x, smoke_steps);
    if (MODE == kCollect) D.count[(size_t)y * P.width + x] = smoke_steps;
    else reinterpret_cast<uchar4 *>(P.out)[(size_t)y * P.width + x] = px4;
#if defined(F3D_SMOKE_TILE_CLOCK)
    const uint64_t clock1 = wall_clock64();  // 100 MHz
    uint32_t *words = reinterpret_cast<uint32_t *>(P.out);
    if (MODE != kCollect && threadIdx.x == 0u) words[(size_t)y * P.width + x] = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)clock0);
    if (MODE != kCollect && threadIdx.x == 1u) words[(size_t)y * P.width + x] = (uint32_t)(clock1 - clock0);
#endif
}
template <uint32_t MODE>
__global__ __launch_bounds__(64) void k_smoke_rays(const SmokeParams P, const Deferred D) {
    extern __shared__ uint32_t wave_chunks_lds[];
    volatile uint32_t *wave_chunks = wave_chunks_lds;
    if (MODE == kCollect) {
        for (uint32_t i = threadIdx.x; i < D.chunks_per_tile; i += 64u) wave_chunks[i] = kUnset;
        if (threadIdx.x == 0u) wave_chunks[D.chunks_per_tile] = 0u;
    }
    uint32_t x, y;
    if (tile_pixel(P, blockIdx.x, threadIdx.x, x, y)) walk_pixel<MODE>(P, D, wave_chunks, x, y);
    if (MODE == kCollect && threadIdx.x == 0u) D.spilled[blockIdx.x] = wave_chunks[D.chunks_per_tile];
}

// The self-shadow marches of the listed steps: a lane per slot, a wave per row of a chunk, the waves of the launch striding
// over the rows of the chunks that k_smoke_rays<kCollect> handed out (their number is on the device: no host round trip).
__global__ __launch_bounds__(64) void k_smoke_light(const SmokeParams P, const Deferred D) {
    const uint32_t rows = min(*D.cursor, D.capacity) * kChunkRows, lane = threadIdx.x & 63u;
    const SmokeBox box = smoke_box(P);
    for (uint32_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const uint2 own = D.owner[row / kChunkRows];
        uint32_t x, y;
        if (!tile_pixel(P, own.x, lane, x, y)) continue;
        if (own.y * kChunkRows + row % kChunkRows >= D.count[(size_t)y * P.width + x]) continue;  // the pixel's ray has fewer smoke steps
        const uint32_t slot = row * 64u + lane;
        const float4 p = D.where[slot];
        D.light[slot] = sun_transmittance(P, box, V3{p.x, p.y, p.z});
    }
}

// The radiance of a pixel's listed steps, in their order (march_ray's accumulation, render.rs:237-288).
__global__ __launch_bounds__(64) void k_smoke_shade(const SmokeParams P, const Deferred D) {
    extern __shared__ uint32_t wave_chunks_lds[];
    volatile uint32_t *wave_chunks = wave_chunks_lds;
    for (uint32_t i = threadIdx.x; i < D.chunks_per_tile; i += 64u) wave_chunks[i] = D.chunk_of[(size_t)blockIdx.x * D.chunks_per_tile + i];
    uint32_t x, y;
    if (!tile_pixel(P, blockIdx.x, threadIdx.x, x, y)) return;
    if (D.spilled[blockIdx.x] != 0u) {  // the list ran out under this tile: its rays walked here, with their self-shadow marches
        walk_pixel<kWhole>(P, D, wave_chunks, x, y);
        return;
    }
    const uint32_t count = D.count[(size_t)y * P.width + x], lane = threadIdx.x & 63u;
    float transmittance = 1.0f;
    V3 rgb = V3{0.0f, 0.0f, 0.0f};
    if (count != 0u) {
        V3 origin, dir;
        uint32_t seed;
        pixel_ray(P, x, y, origin, dir, seed);
        const float cos_theta = f_clamp(vdot(dir, P.sun), -1.0f, 1.0f);
        const float g2 = P.st.phase_g * P.st.phase_g;  // henyey_greenstein, as in march_ray
        const float denom = f_max(1.0f + g2 - 2.0f * P.st.phase_g * cos_theta, 1.0e-4f);
        const float phase = (1.0f - g2) / (4.0f * kPi * (denom * f_sqrt(denom)));
        auto slot_of = [&](uint32_t k) { return wave_chunks[k / kChunkRows] * kChunkSlots + (k % kChunkRows) * 64u + lane; };
        uint32_t slot = slot_of(0u);
        float4 where = D.where[slot], fields = D.fields[slot], more = D.more[slot];
        float light = D.light[slot];
        for (uint32_t k = 0u; k < count; k++) {
            const float4 w = where, f = fields, m = more;  // this step; the next one's loads go out before it is evaluated
            const float l = light;
            if (k + 1u < count) {
                slot = slot_of(k + 1u);
                where = D.where[slot];
                fields = D.fields[slot];
                more = D.more[slot];
                light = D.light[slot];
            }
            const float sigma_t = w.w, seg_tr = m.z;
            const float seg_w = sigma_t > 1.0e-6f ? (1.0f - seg_tr) / sigma_t : P.step;
            const V3 source = smoke_source(P, V3{w.x, w.y, w.z}, f.x, f.y, f.z, f.w, m.x, m.y, sigma_t, l, phase);
            rgb = vadd(rgb, vscale(vscale(source, seg_w), transmittance));
            transmittance *= seg_tr;
        }
    }
    reinterpret_cast<uchar4 *>(P.out)[(size_t)y * P.width + x] = smoke_pixel(P, rgb, transmittance);
}

// (Round 5 first built the verdict's prescription -- the pixels that meet smoke sifted into a list, then eight cooperating
// lanes per listed pixel sharing each self-shadow march -- and measured it: bit-identical, 1.65 ms against the one-kernel
// form's 1.46, because it repeats a pixel's primary taps eightfold and spreads a wave's gathers over more cache lines.
// Taking the marches OUT of the ray, above, gives the parallelism without either; the sift form is in the history
// (commit a4420a0 and before), its numbers in profiles/README.md.)

void hip_ok(hipError_t e, const char *what) {
    if (e != hipSuccess) fail(F3D_STATUS_DEVICE, "HIP failure in %s: %s", what, hipGetErrorString(e));
}

V3 normalize_or_zero(V3 a) {  // glam Vec3::normalize_or_zero
    const float rcp = 1.0f / std::sqrt((a.x * a.x) + (a.y * a.y) + (a.z * a.z));
    if (std::isfinite(rcp) && rcp > 0.0f) return V3{a.x * rcp, a.y * rcp, a.z * rcp};
    return V3{0.0f, 0.0f, 0.0f};
}
float len2(V3 a) { return (a.x * a.x) + (a.y * a.y) + (a.z * a.z); }
V3 cross_glam(V3 a, V3 b) { return V3{a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }

void validate_settings(const f3d_smoke_settings &s) {  // SmokeRenderSettings::validate, types.rs:271-316
    const char *names[11] = {"density_scale", "extinction", "scattering", "absorption", "phase_g", "step_size",
                             "shadow_step_size", "jitter_strength", "exposure", "soot_absorption", "fire_glow"};
    const float vals[11] = {s.density_scale, s.extinction, s.scattering, s.absorption, s.phase_g, s.step_size,
                            s.shadow_step_size, s.jitter_strength, s.exposure, s.soot_absorption, s.fire_glow};
    for (int i = 0; i < 11; i++)
        if (!std::isfinite(vals[i])) fail(F3D_STATUS_RENDER, "%s must be finite", names[i]);
    if (s.density_scale < 0.0f || s.extinction < 0.0f || s.scattering < 0.0f)
        fail(F3D_STATUS_RENDER, "density_scale, extinction, and scattering must be >= 0");
    if (s.absorption < 0.0f || s.soot_absorption < 0.0f || s.fire_glow < 0.0f)
        fail(F3D_STATUS_RENDER, "absorption, soot_absorption, and fire_glow must be >= 0");
    if (!(s.phase_g >= -0.99f && s.phase_g <= 0.99f)) fail(F3D_STATUS_RENDER, "phase_g must be in [-0.99, 0.99]");
    if (s.step_size < 0.0f || s.shadow_step_size < 0.0f) fail(F3D_STATUS_RENDER, "step sizes must be >= 0");
    if (s.max_steps == 0u || s.shadow_steps == 0u) fail(F3D_STATUS_RENDER, "max_steps and shadow_steps must be >= 1");
    if (!(s.jitter_strength >= 0.0f && s.jitter_strength <= 1.0f)) fail(F3D_STATUS_RENDER, "jitter_strength must be in [0, 1]");
    for (int c = 0; c < 2; c++)
        for (int a = 0; a < 3; a++) {
            const float v = c ? s.dense_color[a] : s.thin_color[a];
            if (!std::isfinite(v) || v < 0.0f)
                fail(F3D_STATUS_RENDER, "%s[%d] must be finite and >= 0", c ? "dense_color" : "thin_color", a);
        }
}

void validate_volume(const f3d_smoke_volume &v) {  // SmokeDomainConfig::validate, types.rs:29-62
    for (int a = 0; a < 3; a++)
        if (v.dims[a] < 2u) fail(F3D_STATUS_VALUE, "dims[%d] must be >= 2", a);
    const uint64_t n = (uint64_t)v.dims[0] * v.dims[1] * v.dims[2];
    if (n > 256ull * 256ull * 256ull)
        fail(F3D_STATUS_VALUE, "smoke domain has %llu voxels, exceeding CPU reference limit %llu", (unsigned long long)n,
             256ull * 256ull * 256ull);
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(v.voxel_size[a]) || v.voxel_size[a] <= 0.0f) fail(F3D_STATUS_VALUE, "voxel_size[%d] must be finite and > 0", a);
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(v.origin[a])) fail(F3D_STATUS_VALUE, "origin[%d] must be finite", a);
    if (!v.density || !v.temperature || !v.soot || !v.humidity || !v.emission || !v.age)
        fail(F3D_STATUS_VALUE, "all six smoke fields are required");
}

}  // namespace

// ABI-5 shim (one revision): names the stream of the calling thread's DEFAULT context and, with it, opts the thread's
// handle-less calls into returning before their kernels have finished.  New callers hold a sequence handle (below).
extern "C" void f3d_smoke_set_stream(void *stream) {
    SmokeContext &ctx = thread_default_smoke_context();
    ctx.stream = static_cast<hipStream_t>(stream);
    ctx.async_ok = true;
}
extern "C" int f3d_smoke_wait_fields_read(void *stream) {
    SmokeContext &ctx = thread_default_smoke_context();
    if (!ctx.fields_read) return F3D_STATUS_OK;
    return hipStreamWaitEvent(static_cast<hipStream_t>(stream), ctx.fields_read, 0) == hipSuccess ? F3D_STATUS_OK : F3D_STATUS_DEVICE;
}

extern "C" int f3d_smoke_render(const f3d_smoke_volume *vol, const f3d_smoke_view *view, const f3d_smoke_settings *settings,
                                uint8_t *rgba, double *kernel_seconds, char *err, size_t errlen) {
    if (err && errlen) err[0] = 0;
    int rc = F3D_STATUS_OK;
    hipEvent_t e0 = nullptr, e1 = nullptr;  // (destroyed behind the catch blocks: a failure in between must not leak them)
    try {
        if (!vol || !view || !settings || !rgba) fail(F3D_STATUS_VALUE, "null argument");
        validate_settings(*settings);
        validate_volume(*vol);
        if (view->width == 0u || view->height == 0u) fail(F3D_STATUS_RENDER, "width and height must be >= 1");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
            fail(F3D_STATUS_DEVICE, "no HIP device available: libf3dhip has no CPU fallback");
        SmokeParams P{};
        P.nx = vol->dims[0];
        P.ny = vol->dims[1];
        P.nz = vol->dims[2];
        P.origin = V3{vol->origin[0], vol->origin[1], vol->origin[2]};
        P.voxel = V3{vol->voxel_size[0], vol->voxel_size[1], vol->voxel_size[2]};
        P.bmin = P.origin;
        P.bmax = V3{vol->origin[0] + (float)vol->dims[0] * vol->voxel_size[0], vol->origin[1] + (float)vol->dims[1] * vol->voxel_size[1],
                    vol->origin[2] + (float)vol->dims[2] * vol->voxel_size[2]};
        P.frame_index = vol->frame_index;
        P.width = view->width;
        P.height = view->height;
        P.mode = view->projection ? 1u : 0u;
        P.sun = normalize_or_zero(V3{view->sun_direction[0], view->sun_direction[1], view->sun_direction[2]});
        if (P.mode == 0u) {
            if (!std::isfinite(view->fovy_deg) || view->fovy_deg <= 0.0f || view->fovy_deg >= 179.0f)
                fail(F3D_STATUS_RENDER, "fovy_deg must be finite and in (0, 179)");
            P.eye = V3{view->camera_pos[0], view->camera_pos[1], view->camera_pos[2]};
            const V3 target = V3{view->target[0], view->target[1], view->target[2]};
            P.forward = normalize_or_zero(V3{target.x - P.eye.x, target.y - P.eye.y, target.z - P.eye.z});
            if (len2(P.forward) < 1.0e-12f) fail(F3D_STATUS_RENDER, "camera_pos and target must not be equal");
            const V3 up = normalize_or_zero(V3{view->up[0], view->up[1], view->up[2]});
            if (len2(up) < 1.0e-12f) fail(F3D_STATUS_RENDER, "up vector must not be zero");
            P.right = normalize_or_zero(cross_glam(P.forward, up));
            P.camera_up = normalize_or_zero(cross_glam(P.right, P.forward));
            if (len2(P.sun) < 1.0e-12f) fail(F3D_STATUS_RENDER, "sun_direction must not be zero");
            P.tan_half_fov = std::tan((view->fovy_deg * (3.14159265358979323846f / 180.0f)) * 0.5f);
            P.aspect = (float)view->width / (float)view->height;
        } else {
            P.view = normalize_or_zero(V3{view->view_direction[0], view->view_direction[1], view->view_direction[2]});
            if (len2(P.view) < 1.0e-12f) fail(F3D_STATUS_RENDER, "view_direction must not be zero");
            if (len2(P.sun) < 1.0e-12f) fail(F3D_STATUS_RENDER, "sun_direction must not be zero");
        }
        const float min_step = std::fmax(std::fmin(std::fmin(std::fmin(INFINITY, vol->voxel_size[0]), vol->voxel_size[1]), vol->voxel_size[2]), 1.0e-4f);
        P.step = settings->step_size > 0.0f ? settings->step_size : min_step * 0.75f;
        P.shadow_step = settings->shadow_step_size > 0.0f ? settings->shadow_step_size : P.step * 2.0f;
        const V3 ext = V3{P.bmax.x - P.bmin.x, P.bmax.y - P.bmin.y, P.bmax.z - P.bmin.z};
        P.diagonal = std::fmax(std::sqrt(len2(ext)), P.step * 2.0f);
        P.st = SmokeSettingsDev{settings->density_scale, settings->extinction, settings->scattering, settings->absorption,
                                settings->phase_g, settings->max_steps, settings->self_shadow ? 1u : 0u, settings->shadow_steps,
                                settings->jitter_strength, settings->exposure, settings->soot_absorption, settings->fire_glow,
                                V3{settings->thin_color[0], settings->thin_color[1], settings->thin_color[2]},
                                V3{settings->dense_color[0], settings->dense_color[1], settings->dense_color[2]}};

        std::lock_guard<std::mutex> workspace_guard(workspace_lock());  // one smoke call at a time enqueues (f3d_devmem.h)
        uint32_t n_scratch = 0;
        auto alloc = [&](size_t bytes, const char *what) {  // stream-ordered scratch that stays for the next call
            char tag[48];
            snprintf(tag, sizeof(tag), "smoke.render.%u", n_scratch++);  // (the same sequence of requests in every call)
            void *p = nullptr;
            hip_ok(workspace(&p, tag, bytes), what);
            return p;
        };
        const uint64_t n = (uint64_t)P.nx * P.ny * P.nz;
        const float *host[6] = {vol->density, vol->temperature, vol->soot, vol->humidity, vol->emission, vol->age};
        const float *dev[6];
        for (int i = 0; i < 6; i++) {  // a field that already is device memory (a resident smoke sequence) is read where it is
            hipPointerAttribute_t attr{};
            const bool resident = hipPointerGetAttributes(&attr, host[i]) == hipSuccess && attr.type == hipMemoryTypeDevice;
            (void)hipGetLastError();
            if (resident) {
                dev[i] = host[i];
                n_scratch++;  // (keeps the numbering of the requests after it)
                continue;
            }
            float *up = (float *)alloc(n * sizeof(float), "smoke field");
            hip_ok(hipStreamSynchronize(call_stream()), "smoke field upload");  // (whatever the stream still reads from the buffer)
            hip_ok(hipMemcpy(up, host[i], n * sizeof(float), hipMemcpyHostToDevice), "smoke field upload");
            dev[i] = up;
        }
        float4 *rec_a = (float4 *)alloc(n * sizeof(float4), "smoke records");
        float2 *rec_b = (float2 *)alloc(n * sizeof(float2), "smoke records");
        P.ocx = ((P.nx - 1u) >> kOccShift) + 1u;
        P.ocy = ((P.ny - 1u) >> kOccShift) + 1u;
        const size_t occ_bytes = (size_t)P.ocx * P.ocy * (((P.nz - 1u) >> kOccShift) + 1u);
        uint8_t *occupied = (uint8_t *)alloc(occ_bytes, "smoke empty-space map");
        hip_ok(hipMemsetAsync(occupied, 0, occ_bytes, call_stream()), "smoke empty-space map");
        P.occupied = occupied;
        const PackParams pack{dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], rec_a, rec_b, n, occupied, P.nx, P.ny, P.nz, P.ocx, P.ocy};
        hipLaunchKernelGGL(k_smoke_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, call_stream(), pack);
        hip_ok(hipGetLastError(), "smoke pack kernel");
        uint32_t *bounds = (uint32_t *)alloc(6 * sizeof(uint32_t), "smoke bounds");
        const uint32_t n_slices = ((P.nz - 1u) >> kOccShift) + 1u;
        uint4 *slices = (uint4 *)alloc((size_t)n_slices * sizeof(uint4), "smoke bounds");
        hipLaunchKernelGGL(k_smoke_bounds, dim3(n_slices), dim3(256), 0, call_stream(), occupied, P.ocx, P.ocy, slices);
        hipLaunchKernelGGL(k_smoke_bounds_fold, dim3(1), dim3(64), 0, call_stream(), slices, n_slices, bounds);
        hip_ok(hipGetLastError(), "smoke bounds kernel");
        if (!fields_read_event()) hip_ok(hipEventCreateWithFlags(&fields_read_event(), hipEventDisableTiming), "event");
        hip_ok(hipEventRecord(fields_read_event(), call_stream()), "event");  // the volume's fields are not read after this point
        P.bounds = bounds;
        P.clip = 1u;
        P.known_div = 1u;
        for (int a = 0; a < 3; a++) {
            const float d = vol->voxel_size[a];
            if (!(d > 0.0f) || !std::isfinite(d) || !std::isfinite(vol->origin[a])) P.clip = 0u;
            if (!div_known_divisor(d)) P.known_div = 0u;
        }
        P.voxel_rcp = V3{1.0f / P.voxel.x, 1.0f / P.voxel.y, 1.0f / P.voxel.z};  // IEEE divisions: correctly rounded
        P.rec_a = rec_a;
        P.rec_b = rec_b;
        const size_t px = (size_t)P.width * P.height;
        hipPointerAttribute_t out_attr{};
        const bool out_on_device = hipPointerGetAttributes(&out_attr, rgba) == hipSuccess && out_attr.type == hipMemoryTypeDevice;
        (void)hipGetLastError();
        P.out = out_on_device ? rgba : (uint8_t *)alloc(px * 4, "smoke rgba");  // (a device image stays on the device: the composite reads it there)
        if (out_on_device) n_scratch++;
        // a device image whose caller does not ask for the kernel time: the call returns with its launches enqueued
        const bool timed = kernel_seconds != nullptr || !out_on_device || !current_smoke_context()->async_ok;
        if (timed) {
            hip_ok(hipEventCreate(&e0), "event");
            hip_ok(hipEventCreate(&e1), "event");
            hip_ok(hipEventRecord(e0, call_stream()), "event");
        }
        const uint32_t tiles = ((P.width + 7u) / 8u) * ((P.height + 7u) / 8u);
        const char *form = getenv("F3D_SMOKE_MARCH");
        Deferred D{};
        D.chunks_per_tile = (P.st.max_steps + kChunkRows - 1u) / kChunkRows;
        bool deferred = P.st.self_shadow != 0u && !form && D.chunks_per_tile <= 4096u;
        if (deferred) {  // the default: the self-shadow marches as a launch of their own between two walks of the rays
            // The list of deferred steps, 52 B a slot: kListStepsPerPixel in-volume steps of every pixel (a tile takes them in
            // chunks of 16 steps x 64 lanes), capped at F3D_SMOKE_SHADOW_MB.  A tile whose steps do not fit is walked by
            // k_smoke_shade in the one-kernel form (same result), and a list that cannot be allocated at all sends the whole
            // frame there.  f3d_smoke_seq_stats reports how much of it a render used.
            size_t slots = std::max<size_t>((size_t)1 << 20, px * kListStepsPerPixel);
            const size_t cap_mb = getenv("F3D_SMOKE_SHADOW_MB") ? (size_t)strtoull(getenv("F3D_SMOKE_SHADOW_MB"), nullptr, 10) : kListCapMb;
            slots = std::min<size_t>(slots, std::max<size_t>((cap_mb << 20) / 52u, kChunkSlots));
            if (const char *e = getenv("F3D_SMOKE_SHADOW_SLOTS")) slots = (size_t)strtoull(e, nullptr, 10);  // test hook: a list that runs out
            D.capacity = (uint32_t)std::min<size_t>(std::max<size_t>(slots / kChunkSlots, 1u), 1u << 21);
            bool out_of_memory = false;
            auto named = [&](const char *tag, size_t bytes) -> void * {  // (requests of this form only: their own tags)
                void *q = nullptr;
                if (out_of_memory) return q;
                const hipError_t e = getenv("F3D_SMOKE_SHADOW_OOM") ? hipErrorOutOfMemory : workspace(&q, tag, bytes);  // (test hook)
                if (e == hipErrorOutOfMemory) {
                    (void)hipGetLastError();
                    out_of_memory = true;
                    return nullptr;
                }
                hip_ok(e, "smoke shadow list");
                return q;
            };
            const size_t list = (size_t)D.capacity * kChunkSlots;
            D.where = (float4 *)named("smoke.render.shadow.where", list * sizeof(float4));
            D.fields = (float4 *)named("smoke.render.shadow.fields", list * sizeof(float4));
            D.more = (float4 *)named("smoke.render.shadow.more", list * sizeof(float4));
            D.light = (float *)named("smoke.render.shadow.light", list * sizeof(float));
            D.spilled = (uint32_t *)named("smoke.render.shadow.spilled", (size_t)tiles * sizeof(uint32_t));
            D.chunk_of = (uint32_t *)named("smoke.render.shadow.chunk_of", (size_t)tiles * D.chunks_per_tile * sizeof(uint32_t));
            D.owner = (uint2 *)named("smoke.render.shadow.owner", (size_t)D.capacity * sizeof(uint2));
            D.count = (uint32_t *)named("smoke.render.shadow.count", px * sizeof(uint32_t));
            D.cursor = (uint32_t *)named(kShadowCursorTag, sizeof(uint32_t));
            if (out_of_memory) deferred = false;  // the one-kernel form needs no list
        }
        current_smoke_context()->shadow_capacity = deferred ? D.capacity : 0u;
        if (deferred) {
            hip_ok(hipMemsetAsync(D.cursor, 0, sizeof(uint32_t), call_stream()), "smoke shadow list");
            const size_t lds = ((size_t)D.chunks_per_tile + 1u) * sizeof(uint32_t);
            hipLaunchKernelGGL(k_smoke_rays<kCollect>, dim3(tiles), dim3(64), lds, call_stream(), P, D);
            static const unsigned light_waves = getenv("F3D_SMOKE_LIGHT_WAVES") ? (unsigned)atoi(getenv("F3D_SMOKE_LIGHT_WAVES")) : 16384u;  // (experiment switch)
            hipLaunchKernelGGL(k_smoke_light, dim3(light_waves), dim3(64), 0, call_stream(), P, D);
            hipLaunchKernelGGL(k_smoke_shade, dim3(tiles), dim3(64), lds, call_stream(), P, D);
        } else {  // one lane per pixel, the whole ray (F3D_SMOKE_MARCH=single, or no self-shadowing)
            hipLaunchKernelGGL(k_smoke_rays<kWhole>, dim3(tiles), dim3(64), 0, call_stream(), P, D);
        }
        hip_ok(hipGetLastError(), "smoke kernel");
        if (timed) {
            hip_ok(hipEventRecord(e1, call_stream()), "event");
            if (out_on_device) hip_ok(hipEventSynchronize(e1), "smoke kernel");
            else {
                hip_ok(hipEventSynchronize(e1), "smoke kernel");  // (the copy below is not ordered behind a stream of the caller's)
                hip_ok(hipMemcpy(rgba, P.out, px * 4, hipMemcpyDeviceToHost), "smoke readback");
            }
            float ms = 0.0f;
            (void)hipEventElapsedTime(&ms, e0, e1);
            if (kernel_seconds) *kernel_seconds = ms * 1e-3;
        }
    } catch (const Failure &f) {
        rc = report(f, err, errlen);
    } catch (const std::exception &e) {
        if (err && errlen) snprintf(err, errlen, "host failure: %s", e.what());
        rc = F3D_STATUS_DEVICE;
    } catch (...) {
        rc = F3D_STATUS_DEVICE;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return rc;
}

// ---- sequence handle (ABI 6) ----------------------------------------------------------------------------------------------
// A resident smoke sequence as an object: its two streams (solver, marcher), the ordering between them, its scratch and the
// event that marks "the marcher has read the fields" all belong to the handle.  Round 5 kept the stream and the event in
// thread-local variables behind f3d_smoke_set_stream / f3d_smoke_wait_fields_read: the library "remembered the last render of
// the thread", and a caller driving two sequences had to re-name its stream before every call.  (No counterpart in the
// reference, whose solver and marcher are host loops: src/smoke/sim.rs, src/smoke/render.rs.)
struct f3d_smoke_seq {
    int device = 0;
    hipStream_t solver = nullptr, march = nullptr;  // the caller's streams (NULL: the null stream); they outlive the handle
    hipEvent_t stepped = nullptr;  // the last step's launches, on the solver's stream
    bool has_stepped = false;
    SmokeContext ctx;
};

namespace {
std::atomic<unsigned long long> g_smoke_seq_ids{1ull};

struct SeqDevice {  // the handle's device for the duration of a call
    int prev = -1;
    explicit SeqDevice(int device) {
        (void)hipGetDevice(&prev);
        if (prev != device) (void)hipSetDevice(device);
        else prev = -1;
    }
    ~SeqDevice() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};
int seq_fail(char *err, size_t errlen, int status, const char *what) {
    if (err && errlen) snprintf(err, errlen, "%s", what);
    return status;
}
}  // namespace

extern "C" int f3d_smoke_seq_create(void *stream_solver, void *stream_march, f3d_smoke_seq **out, char *err, size_t errlen) {
    if (err && errlen) err[0] = 0;
    if (!out) return seq_fail(err, errlen, F3D_STATUS_VALUE, "null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return seq_fail(err, errlen, F3D_STATUS_DEVICE, "no HIP device available: libf3dhip has no CPU fallback");
    f3d_smoke_seq *q = new (std::nothrow) f3d_smoke_seq();
    if (!q) return seq_fail(err, errlen, F3D_STATUS_DEVICE, "out of host memory");
    bool ok = hipGetDevice(&q->device) == hipSuccess;
    q->solver = static_cast<hipStream_t>(stream_solver);
    q->march = static_cast<hipStream_t>(stream_march);
    ok = ok && hipEventCreateWithFlags(&q->stepped, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&q->ctx.fields_read, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        if (q->stepped) (void)hipEventDestroy(q->stepped);
        if (q->ctx.fields_read) (void)hipEventDestroy(q->ctx.fields_read);
        delete q;
        return seq_fail(err, errlen, F3D_STATUS_DEVICE, "could not create the sequence's events");
    }
    q->ctx.id = g_smoke_seq_ids.fetch_add(1ull);
    q->ctx.async_ok = true;
    // (a fresh fields_read event has never been recorded: waiting for it returns at once, as it should before the first render)
    *out = q;
    return F3D_STATUS_OK;
}

extern "C" void f3d_smoke_seq_destroy(f3d_smoke_seq *q) {
    if (!q) return;
    SeqDevice guard(q->device);
    (void)hipStreamSynchronize(q->solver);
    (void)hipStreamSynchronize(q->march);
    char suffix[40];
    snprintf(suffix, sizeof(suffix), "#%llu", q->ctx.id);
    workspace_release(suffix);  // the scratch of this sequence goes back (to the library's pool; f3d_device_pool_trim empties that)
    (void)hipEventDestroy(q->stepped);
    (void)hipEventDestroy(q->ctx.fields_read);
    delete q;
}

extern "C" int f3d_smoke_seq_streams(f3d_smoke_seq *q, void **stream_solver, void **stream_march) {
    if (!q) return F3D_STATUS_VALUE;
    if (stream_solver) *stream_solver = q->solver;
    if (stream_march) *stream_march = q->march;
    return F3D_STATUS_OK;
}

extern "C" int f3d_smoke_step(f3d_smoke_state *, const f3d_smoke_step_settings *, const f3d_smoke_emitter *, uint32_t, uint32_t, double *, char *, size_t);
extern "C" int f3d_smoke_composite(const f3d_composite_desc *, uint8_t *, double *, char *, size_t);

// `steps` solver steps on the solver's stream, behind the last render's reads of the fields.
extern "C" int f3d_smoke_seq_step(f3d_smoke_seq *q, f3d_smoke_state *state, const f3d_smoke_step_settings *settings, const f3d_smoke_emitter *emitters,
                                  uint32_t emitter_count, uint32_t steps, double *device_seconds, char *err, size_t errlen) {
    if (!q) return seq_fail(err, errlen, F3D_STATUS_VALUE, "null sequence handle");
    SeqDevice guard(q->device);
    q->ctx.stream = q->solver;
    if (hipStreamWaitEvent(q->solver, q->ctx.fields_read, 0) != hipSuccess) return seq_fail(err, errlen, F3D_STATUS_DEVICE, "could not order the step behind the last render");
    ScopedSmokeContext scope(&q->ctx);
    const int rc = f3d_smoke_step(state, settings, emitters, emitter_count, steps, device_seconds, err, errlen);
    if (rc == F3D_STATUS_OK) {
        if (hipEventRecord(q->stepped, q->solver) != hipSuccess) return seq_fail(err, errlen, F3D_STATUS_DEVICE, "could not record the step");
        q->has_stepped = true;
    }
    return rc;
}

// The march of the volume into `rgba` on the marcher's stream, behind the last step.
extern "C" int f3d_smoke_seq_render(f3d_smoke_seq *q, const f3d_smoke_volume *volume, const f3d_smoke_view *view, const f3d_smoke_settings *settings,
                                    uint8_t *rgba, double *kernel_seconds, char *err, size_t errlen) {
    if (!q) return seq_fail(err, errlen, F3D_STATUS_VALUE, "null sequence handle");
    SeqDevice guard(q->device);
    q->ctx.stream = q->march;
    if (q->has_stepped && hipStreamWaitEvent(q->march, q->stepped, 0) != hipSuccess)
        return seq_fail(err, errlen, F3D_STATUS_DEVICE, "could not order the render behind the last step");
    ScopedSmokeContext scope(&q->ctx);
    return f3d_smoke_render(volume, view, settings, rgba, kernel_seconds, err, errlen);  // (records ctx.fields_read behind its pack kernels)
}

// The composite on the marcher's stream (behind the render whose layer it reads).
extern "C" int f3d_smoke_seq_composite(f3d_smoke_seq *q, const f3d_composite_desc *desc, uint8_t *out_rgba, double *kernel_seconds, char *err, size_t errlen) {
    if (!q) return seq_fail(err, errlen, F3D_STATUS_VALUE, "null sequence handle");
    SeqDevice guard(q->device);
    q->ctx.stream = q->march;
    ScopedSmokeContext scope(&q->ctx);
    return f3d_smoke_composite(desc, out_rgba, kernel_seconds, err, errlen);
}

// What the sequence holds and how much of the deferred self-shadow list its last render used (waits for that render).
extern "C" int f3d_smoke_seq_stats(f3d_smoke_seq *q, f3d_smoke_seq_stats_t *out, char *err, size_t errlen) {
    if (!q || !out) return seq_fail(err, errlen, F3D_STATUS_VALUE, "null argument");
    SeqDevice guard(q->device);
    char suffix[40];
    snprintf(suffix, sizeof(suffix), "#%llu", q->ctx.id);
    out->scratch_bytes = workspace_bytes(suffix);
    out->shadow_list_chunks = 0u;
    out->shadow_list_chunks_used = 0u;
    out->shadow_list_slots_per_chunk = kChunkSlots;
    if (q->ctx.shadow_capacity != 0u) {
        // the fill count by name, under the lock: f3d_device_pool_trim may have freed the list since the render (then: no list)
        std::lock_guard<std::mutex> lock(workspace_lock());
        if (const void *cursor = workspace_find(q->device, kShadowCursorTag, suffix)) {
            if (hipStreamSynchronize(q->march) != hipSuccess) return seq_fail(err, errlen, F3D_STATUS_DEVICE, "the marcher's stream failed");
            uint32_t used = 0u;
            if (hipMemcpy(&used, cursor, sizeof(used), hipMemcpyDeviceToHost) != hipSuccess) return seq_fail(err, errlen, F3D_STATUS_DEVICE, "could not read the list's fill count");
            out->shadow_list_chunks = q->ctx.shadow_capacity;
            out->shadow_list_chunks_used = used;  // (may exceed the capacity: that many were asked for; the excess was walked in the one-kernel form)
        }
    }
    return F3D_STATUS_OK;
}
