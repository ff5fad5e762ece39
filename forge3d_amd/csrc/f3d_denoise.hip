// forge3d_amd/csrc/f3d_denoise.hip -- edge-aware a-trous denoiser on the GPU.
//
// Reference: the public `forge3d.denoise.atrous_denoise` (python/forge3d/denoise.py:18-127), a pure
// NumPy post filter over a finished render, guided by the albedo / normal / depth AOVs the terrain
// path tracer returns.  Semantics restated in oracle/denoise_oracle.py (which reproduces the
// reference's outputs bit for bit); here one gather kernel per pass:
//   * 5x5 taps at spacing 1, 2, 4, ... with B3-spline weights [1,4,6,4,1]/16 per axis        (:74-90)
//   * taps outside the image read ZERO for the colour and for every guide and still add their
//     weight to the normaliser (the reference's zero-padded `_shift`, :130-151)
//   * weight = base * exp(-|dg|^2 / D_color) [* exp(-|dg|^2 / D_albedo)] * exp(-acos(n.n')^2 / D_normal)
//     * exp(-dd^2 / D_depth),  D_x = f32(2 sigma_x^2 + 1e-8)                                 (:98-119)
//   * out = sum(colour * w) / max(sum(w), 1e-8)                                               (:121-124)
// The arithmetic lives in f3d_denoise.h (host and device; tests/denoise_host runs it on the CPU); the kernels here only find
// their pixel.  Non-finite inputs follow NumPy's clip / maximum (a NaN normal gives NaN pixels, f3d_denoise.h); the tap spacing
// saturates at 2^28, so 32 passes and more are defined.
// Parity: against tests/denoise_reference.py, a float64 statement of the above that also covers the calls
// the reference refuses (a shift between one and two image sizes), per parameter set within 4 x the float32 oracle's own
// distance from float64 -- recorded in denoise_reference.py; measured on MI355X: 3.6e-7 with all guides at the default sigmas
// (gate 1.6e-6), 2.3e-6 colour-only over 40 passes (9.2e-6), 2.7e-5 at sigmas of 0.01 / 0.02 (1.1e-4): the device is as far
// from float64 as NumPy's float32 is.  And, as before, |hip - reference| <= 2e-5 on the committed vectors
// (tests/golden/atrous_cases.npz, written by the reference's own implementation).  HBM/L2-bound gather: 25 taps x up to 40 B
// per pixel and pass, neighbouring threads read neighbouring texels at every spacing.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/f3d_terrain_pt.h"
#include "f3d_denoise.h"
#include "f3d_devmem.h"

namespace {

using namespace f3d;

__global__ void k_normalize(const float *in, float *out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    atrous_normalize(in, out, i);
}

__global__ __launch_bounds__(256) void k_atrous(const AtrousParams P) {
    const int x = (int)(blockIdx.x * blockDim.x + threadIdx.x), y = (int)(blockIdx.y * blockDim.y + threadIdx.y);
    if (x >= (int)P.width || y >= (int)P.height) return;
    atrous_pixel(P, x, y);
}

struct DeviceBuffers {
    std::vector<void *> owned;
    ~DeviceBuffers() {
        for (void *p : owned) (void)f3d::device_free(p);
    }
    float *upload(const float *host, size_t floats, std::string &why) {
        void *p = nullptr;
        if (f3d::device_alloc(&p, floats * sizeof(float)) != hipSuccess) {
            why = "device allocation failed";
            return nullptr;
        }
        owned.push_back(p);
        if (host && hipMemcpy(p, host, floats * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
            why = "upload failed";
            return nullptr;
        }
        return (float *)p;
    }
};

int fail(int status, const char *msg, char *err, size_t errlen) {
    if (err && errlen) snprintf(err, errlen, "%s", msg);
    return status;
}

}  // namespace

extern "C" int f3d_atrous_denoise(const float *color, const float *albedo, const float *normal, const float *depth,
                                  uint32_t width, uint32_t height, int32_t iterations, float sigma_color,
                                  float sigma_albedo, float sigma_normal, float sigma_depth, float *out, char *err,
                                  size_t errlen) {
    if (!color || !out || width == 0 || height == 0)
        return fail(F3D_STATUS_VALUE, "color must be (H, W, 3)", err, errlen);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(F3D_STATUS_DEVICE, "no HIP device available: libf3dhip has no CPU fallback", err, errlen);
    const size_t px = (size_t)width * height;
    DeviceBuffers dev;
    std::string why;
    float *d_color = dev.upload(color, 3 * px, why);
    float *d_a = d_color ? dev.upload(nullptr, 3 * px, why) : nullptr;
    float *d_b = d_a ? dev.upload(nullptr, 3 * px, why) : nullptr;
    float *d_albedo = (d_b && albedo) ? dev.upload(albedo, 3 * px, why) : nullptr;
    float *d_normal_raw = (d_b && normal) ? dev.upload(normal, 3 * px, why) : nullptr;
    float *d_normal = (d_b && normal) ? dev.upload(nullptr, 3 * px, why) : nullptr;
    float *d_depth = (d_b && depth) ? dev.upload(depth, px, why) : nullptr;
    if (!d_b || (albedo && !d_albedo) || (normal && (!d_normal_raw || !d_normal)) || (depth && !d_depth))
        return fail(F3D_STATUS_DEVICE, why.empty() ? "device allocation failed" : why.c_str(), err, errlen);
    if (normal) hipLaunchKernelGGL(k_normalize, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, nullptr, d_normal_raw, d_normal, (uint32_t)px);

    AtrousParams P = atrous_params(albedo ? d_albedo : d_color, d_normal, d_depth, width, height, albedo != nullptr, sigma_color, sigma_albedo,
                                   sigma_normal, sigma_depth);
    const int passes = atrous_passes(iterations);
    const float *src = d_color;
    float *dst = d_a;
    const dim3 block(16, 16), grid((width + 15) / 16, (height + 15) / 16);
    for (int i = 0, step = 1; i < passes; i++, step = atrous_next_step(step)) {
        P.src = src;
        P.dst = dst;
        P.step = step;
        hipLaunchKernelGGL(k_atrous, grid, block, 0, nullptr, P);
        src = dst;
        dst = dst == d_a ? d_b : d_a;
    }
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return fail(F3D_STATUS_DEVICE, "a-trous kernel failed", err, errlen);
    if (hipMemcpy(out, src, 3 * px * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(F3D_STATUS_DEVICE, "read-back failed", err, errlen);
    return F3D_STATUS_OK;
}
