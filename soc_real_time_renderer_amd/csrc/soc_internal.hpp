// soc_internal.hpp — host-side helpers shared by the C-ABI entry points (not part of the ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../include/soc_rt.h"
#include "soc_device.hpp"

namespace soc {

// Per-thread last error (soc_last_error_string).
int set_error(int code, const char* fmt, ...);
void clear_error();

inline int bytes_per_pixel(int fmt) {
    switch (fmt) {
    case SOC_FMT_RGBA16F: return 8;
    case SOC_FMT_D32F: return 4;
    case SOC_FMT_R8_UNORM: return 1;
    case SOC_FMT_RGBA8_UNORM:
    case SOC_FMT_RGBA8_SRGB: return 4;
    case SOC_FMT_RGBA32F: return 16;
    default: return 0;
    }
}

inline bool img_ok(const soc_img& im) {
    int b = bytes_per_pixel(im.format);
    return im.data != nullptr && im.width > 0 && im.height > 0 && b > 0 && im.pitch_bytes >= im.width * b;
}

// Validates `im` (and its format when fmt > 0); sets the error string on failure.
int check_img(const soc_img& im, int fmt, const char* pass, const char* what);

// Base address and pitch are multiples of n bytes (a power of two): rows take n-byte loads and stores.
inline bool aligned_to(const soc_img& im, unsigned n) {
    return (reinterpret_cast<uintptr_t>(im.data) & (n - 1)) == 0 && ((unsigned)im.pitch_bytes & (n - 1)) == 0;
}
// The image fits a buffer resource's 32-bit offsets (a signed 24-bit row x pitch product).
inline bool buffer_range_ok(const soc_img& im) {
    return (long long)im.pitch_bytes * im.height < (1ll << 31) && im.pitch_bytes < (1 << 23);
}

inline DImg dimg(const soc_img& im) { return DImg{static_cast<char*>(im.data), im.width, im.height, im.pitch_bytes}; }

inline Mat4 mat4(const float* m) {
    Mat4 r;
    for (int i = 0; i < 16; ++i) r.m[i] = m[i];
    return r;
}

inline hipStream_t hs(soc_stream s) { return reinterpret_cast<hipStream_t>(s); }

// Integer tuning knob from the environment (`dflt` when unset), read once and cached until soc_tuning_reload():
// only the variants the identity tests switch (SOC_SWZ_SSAO, SOC_SSAO_TILE, SOC_TAA_NBR, SOC_COMP_NT, SOC_GB_TEX_PAIRS,
// SOC_CLOUDS_ATMOS_POS, SOC_RENDERER_SSAO_FIRST, SOC_CLOUDS_OD_LUT) and the variants under measurement (SOC_GB_WAVE) are
// knobs; measured-and-rejected variants are removed.
int tuning_knob(const char* name, int dflt);
// Changes with every soc_tuning_reload() (never 0): a launcher on a frame's critical path keeps its block of knobs until
// this moves, instead of one locked lookup by name per knob and call (the clouds planner, clouds_plan.cpp).
uint32_t tuning_generation();
// RN(1 / n) for div_rn (soc_device.hpp), or 0 when n is outside the exhaustively checked range (1..16384).
inline float recip_rn(int n) {
    return n >= 1 && n <= 16384 ? 1.0f / (float)n : 0.0f;
}

// `out` into a caller's buffer (truncated to cap - 1 characters and terminated; none when !buf or !cap): its full length.
int64_t copy_text(const std::string& out, char* buf, size_t cap);

// Checks the launch that was just issued (and a block shape launch() rejected: SOC_E_INVALID_ARG).
int check_launch(const char* pass);

// Launch geometry. Every kernel's flat work-group bound (its __launch_bounds__ / amdgpu_flat_work_group_size) is a
// named constant (kWorkgroup, kSunvisLanes, kSsaoTileLanes, kTaaLdsLanes, kThreads, kBins) that its launcher passes to
// launch() as `bound`. A block of more lanes than the bound, or of none, is not launched: the host records
// SOC_E_INVALID_ARG naming the kernel and the launcher's check_launch returns it, before any HIP call (a launch over
// the bound would otherwise fail on the device as "unspecified launch failure").
bool block_fits(const char* kernel, int bound, dim3 block);
template <typename... P, typename... A>
inline void launch(const char* kernel, int bound, void (*k)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s,
                   A&&... args) {
    if (!block_fits(kernel, bound, block)) return;
    k<<<grid, block, lds, s>>>(static_cast<P>(args)...);
}

inline unsigned ceil_div(unsigned a, unsigned b) { return (a + b - 1) / b; }

// Host fp32 restatements shared with the tone-mapping launcher (bit-identical to the oracle's
// float code: compiled without FMA contraction).
void agx_matrices(float compression, float M[9], float Minv[9]);
void mat4_mul_host(float out[16], const float a[16], const float b[16]);

// The device record of a frame's light ranges (soc_upload_light_bounds writes it, composition.hip reads it; the library's
// own layout, SOC_LIGHT_BOUNDS_DEVICE_BYTES): per light RN(1 / RN(r * r)) for the window (0: unlimited) and RN(r * r) for
// the cull (0: unlimited). A range whose square's reciprocal leaves fp32 is stored as the nearest finite / normal value.
struct LightBoundsDev {
    float point_inv_r2[SOC_MAX_POINT_LIGHTS], spot_inv_r2[SOC_MAX_SPOT_LIGHTS];
    float point_r2[SOC_MAX_POINT_LIGHTS], spot_r2[SOC_MAX_SPOT_LIGHTS];
};
static_assert(sizeof(LightBoundsDev) == SOC_LIGHT_BOUNDS_DEVICE_BYTES, "soc_rt.h states the device record's size");
// A bounded Composition launch: the record, SOC_LIGHTS_* flags and the optional per-wave counter of lights run.
struct LightBoundsCall {
    const void* d_bounds;
    uint32_t flags;
    uint32_t* d_shaded_pairs;
};

// A soc_sun_cascades record (and, when given, its atlas) against soc_rt.h's rules, on the host: SOC_E_INVALID_ARG naming
// the field, with `pass` in front (host_math.cpp).
int check_sun_cascades(const soc_sun_cascades* c, const soc_img* atlas, const char* pass);
// The fused pair path applies to these images at the globals' resolution (composition_plan.cpp; the Composition call
// itself is composition_plan.hpp's record).
bool composition_pair_applicable(const soc_globals* g, const soc_img& target, const soc_img& albedo,
                                 const soc_img& emissive, const soc_img& normal, const soc_img& depth,
                                 const soc_img& clouds);
// The sky pixels of the colour image (depth == 1 -> clouds texel) and their bins into the 8 partial histograms:
// the second-lane half of a Composition run with sky_external.
// soc_cloud_rendering; sky_bound (the render graph's sky lane runs at high priority): the variants that are faster
// only where the sky lane is the frame's critical path (the density grid at twice the resident set, the classification's
// hoisted depth samples). The same bits either way.
// `state`: the renderer-owned record of what the workspace holds between frames (cloud_state.hpp; null: the stateless entry).
struct CloudState;
int cloud_rendering_launch(const soc_globals* g, soc_img depth, soc_img noise, soc_img target, void* workspace,
                           soc_stream stream, bool sky_bound, CloudState* state = nullptr);
int sky_compose_launch(const soc_globals* g, soc_img target, soc_img depth, soc_img clouds, uint32_t* scratch,
                       soc_stream stream);
int histogram_fold_launch(uint32_t* scratch, soc_auto_exposure* ae, soc_stream stream);
// soc_resolve_luminance_histogram that first folds the 8 partial histograms (null: none).
int resolve_luminance_histogram(const soc_globals* g, soc_auto_exposure* ae, uint64_t total_pixels, int32_t wide_accumulator,
                                uint32_t* scratch, soc_stream stream);

}  // namespace soc
