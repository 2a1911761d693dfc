// capi.cpp — host side of the C ABI that every other file leans on: the per-thread error string, the tuning-knob cache,
// the launch checks and the ABI introspection tables. The fp32 restatements are host_math.cpp, the render graph
// render_graph.cpp, the frame scheduler render_execute.cpp.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <mutex>
#include <vector>

#include "soc_internal.hpp"

namespace soc {

static thread_local std::string t_error;

int set_error(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    t_error = buf;
    return code;
}

void clear_error() { t_error.clear(); }

int check_img(const soc_img& im, int fmt, const char* pass, const char* what) {
    if (!img_ok(im))
        return set_error(SOC_E_INVALID_ARG, "%s: %s image invalid (data=%p %dx%d pitch=%d fmt=%d)", pass, what, im.data,
                         im.width, im.height, im.pitch_bytes, im.format);
    if (fmt > 0 && im.format != fmt)
        return set_error(SOC_E_INVALID_ARG, "%s: %s image has format %d, expected %d", pass, what, im.format, fmt);
    // every kernel loads and stores whole texels: the base and the pitch are multiples of the texel size
    const int b = bytes_per_pixel(im.format);
    if (reinterpret_cast<uintptr_t>(im.data) % (uintptr_t)b != 0 || im.pitch_bytes % b != 0)
        return set_error(SOC_E_INVALID_ARG, "%s: %s image is not aligned to its %d-byte texels (data=%p pitch=%d)", pass,
                         what, b, im.data, im.pitch_bytes);
    return SOC_OK;
}

// Tuning knobs: the environment is read once per knob and cached (not per launch);
// soc_tuning_reload() drops the cache so a changed environment takes effect.
namespace {
std::mutex g_knob_mu;
// the environment's value of each knob read so far: (name, (set, value)); a knob that is not set returns the caller's
// default on every call (the default may differ between callers, e.g. per renderer flags)
std::vector<std::pair<std::string, std::pair<bool, int>>> g_knobs;
std::atomic<uint32_t> g_knob_generation{1};   // soc_tuning_reload calls so far, plus one
}  // namespace

uint32_t tuning_generation() { return g_knob_generation.load(std::memory_order_acquire); }

int tuning_knob(const char* name, int dflt) {
    std::lock_guard<std::mutex> lock(g_knob_mu);
    for (const auto& k : g_knobs)
        if (k.first == name) return k.second.first ? k.second.second : dflt;
    const char* e = getenv(name);
    g_knobs.emplace_back(name, std::make_pair(e != nullptr, e ? atoi(e) : 0));
    return e ? atoi(e) : dflt;
}

namespace {
thread_local std::string t_shape_error;   // a block shape launch() rejected since the last check_launch
}  // namespace

bool block_fits(const char* kernel, int bound, dim3 block) {
    const long long lanes = (long long)block.x * block.y * block.z;
    if (lanes >= 1 && lanes <= bound) return true;
    char buf[256];
    std::snprintf(buf, sizeof buf, "%s: block %ux%ux%u (%lld lanes) outside the kernel's launch bound of %d lanes", kernel,
                  block.x, block.y, block.z, lanes, bound);
    if (t_shape_error.empty()) t_shape_error = buf;
    return false;
}

extern "C" int soc_check_block_shape(int32_t bound, int32_t bx, int32_t by, int32_t bz) {
    if (bx < 0 || by < 0 || bz < 0) return set_error(SOC_E_INVALID_ARG, "soc_check_block_shape: negative extent");
    if (!block_fits("soc_check_block_shape", bound, dim3((unsigned)bx, (unsigned)by, (unsigned)bz))) {
        std::string m;
        m.swap(t_shape_error);
        return set_error(SOC_E_INVALID_ARG, "%s", m.c_str());
    }
    return SOC_OK;
}

int check_launch(const char* pass) {
    if (!t_shape_error.empty()) {
        std::string m;
        m.swap(t_shape_error);
        return set_error(SOC_E_INVALID_ARG, "%s: kernel not launched: %s", pass, m.c_str());
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(SOC_E_HIP, "%s: kernel launch failed: %s", pass, hipGetErrorString(e));
    return SOC_OK;
}

}  // namespace soc

using namespace soc;

// =================================================================================================
// ABI introspection
// =================================================================================================
namespace {
struct FieldInfo { const char* type; const char* field; size_t offset; };
#define F(T, f) {#T, #f, offsetof(T, f)}
const FieldInfo kFields[] = {
    F(soc_img, data), F(soc_img, width), F(soc_img, height), F(soc_img, pitch_bytes), F(soc_img, format),
    F(soc_auto_exposure, exposure), F(soc_auto_exposure, histogram_buckets),
    F(soc_sun_info, projection_matrix), F(soc_sun_info, view_matrix), F(soc_sun_info, projection_view_matrix),
    F(soc_sun_info, terrain_y_clip_trick), F(soc_sun_info, position), F(soc_sun_info, direction),
    F(soc_sun_info, exponential_factor), F(soc_sun_info, darkening_factor), F(soc_sun_info, bias), F(soc_sun_info, intensity),
    F(soc_point_light, position), F(soc_point_light, color), F(soc_point_light, intensity),
    F(soc_spot_light, position), F(soc_spot_light, direction), F(soc_spot_light, color), F(soc_spot_light, intensity),
    F(soc_spot_light, cut_off), F(soc_spot_light, outer_cut_off),
    F(soc_camera, position), F(soc_camera, rotation), F(soc_camera, fov_degrees), F(soc_camera, near_clip), F(soc_camera, far_clip),
    F(soc_globals, camera_projection_matrix), F(soc_globals, camera_inverse_projection_matrix),
    F(soc_globals, camera_view_matrix), F(soc_globals, camera_inverse_view_matrix),
    F(soc_globals, camera_projection_view_matrix), F(soc_globals, camera_inverse_projection_view_matrix),
    F(soc_globals, camera_previous_projection_matrix), F(soc_globals, camera_previous_inverse_projection_matrix),
    F(soc_globals, camera_previous_view_matrix), F(soc_globals, camera_previous_inverse_view_matrix),
    F(soc_globals, camera_previous_projection_view_matrix), F(soc_globals, camera_previous_inverse_projection_view_matrix),
    F(soc_globals, jitter), F(soc_globals, previous_jitter), F(soc_globals, camera_position), F(soc_globals, camera_near_clip),
    F(soc_globals, camera_far_clip), F(soc_globals, resolution), F(soc_globals, elapsed_time), F(soc_globals, delta_time),
    F(soc_globals, frame_counter), F(soc_globals, sun_info), F(soc_globals, point_light_count), F(soc_globals, spot_light_count),
    F(soc_globals, point_lights), F(soc_globals, spot_lights), F(soc_globals, terrain_offset), F(soc_globals, terrain_scale),
    F(soc_globals, terrain_height_scale), F(soc_globals, terrain_midpoint), F(soc_globals, terrain_delta),
    F(soc_globals, terrain_min_depth), F(soc_globals, terrain_max_depth), F(soc_globals, terrain_min_tess_level),
    F(soc_globals, terrain_max_tess_level), F(soc_globals, terrain_y_clip_trick), F(soc_globals, terrain_previous_y_clip_trick),
    F(soc_globals, filter_radius), F(soc_globals, ssao_bias), F(soc_globals, ssao_radius), F(soc_globals, ssao_kernel_size),
    F(soc_globals, ambient), F(soc_globals, ambient_occlussion_strength), F(soc_globals, emissive_bloom_strength),
    F(soc_globals, focal_length), F(soc_globals, plane_in_focus), F(soc_globals, aperture), F(soc_globals, adjustment_speed),
    F(soc_globals, log_min_luminance), F(soc_globals, log_max_luminance), F(soc_globals, target_luminance),
    F(soc_globals, saturation), F(soc_globals, agxDs_linear_section), F(soc_globals, peak), F(soc_globals, compression),
    F(soc_frame_images, albedo), F(soc_frame_images, emissive), F(soc_frame_images, normal), F(soc_frame_images, depth),
    F(soc_frame_images, velocity), F(soc_frame_images, shadow), F(soc_frame_images, noise), F(soc_frame_images, bloom_mips),
    F(soc_frame_images, ssao), F(soc_frame_images, ssao_blur), F(soc_frame_images, clouds), F(soc_frame_images, color),
    F(soc_frame_images, history_color), F(soc_frame_images, history_velocity), F(soc_frame_images, output),
    F(soc_frame_images, ssao_noise_table), F(soc_frame_images, auto_exposure), F(soc_frame_images, d_globals),
    F(soc_frame_images, bloom_output), F(soc_frame_images, clouds_workspace),
    F(soc_mesh, positions), F(soc_mesh, normals), F(soc_mesh, uvs), F(soc_mesh, indices), F(soc_mesh, materials),
    F(soc_mesh, vertex_count), F(soc_mesh, triangle_count), F(soc_mesh, model_matrix), F(soc_mesh, normal_matrix),
    F(soc_material, albedo), F(soc_material, emissive), F(soc_material, albedo_factor), F(soc_material, emissive_factor),
    F(soc_material, flags), F(soc_material, has_emissive), F(soc_material, alpha_cutoff), F(soc_material, pad),
    F(soc_material, normal_map),
    F(soc_material, normal_image), F(soc_material, max_anisotropy), F(soc_material, pad2), F(soc_material, paired_texels),
    F(soc_raster_scene, mesh), F(soc_raster_scene, materials), F(soc_raster_scene, material_count),
    F(soc_raster_scene, shadow), F(soc_raster_scene, visibility), F(soc_raster_scene, workspace),
    F(soc_transform, model_matrix), F(soc_transform, normal_matrix),
    F(soc_draw, first_index), F(soc_draw, triangle_count), F(soc_draw, vertex_offset), F(soc_draw, first_vertex),
    F(soc_draw, vertex_count), F(soc_draw, transform), F(soc_draw, material),
    F(soc_draw_scene, positions), F(soc_draw_scene, normals), F(soc_draw_scene, uvs), F(soc_draw_scene, indices),
    F(soc_draw_scene, vertex_count), F(soc_draw_scene, index_count), F(soc_draw_scene, draws), F(soc_draw_scene, draw_count),
    F(soc_draw_scene, transform_count), F(soc_draw_scene, transforms), F(soc_draw_scene, material_count),
    F(soc_draw_scene, pad), F(soc_draw_scene, workspace),
    F(soc_terrain_layer, mesh), F(soc_terrain_layer, shadow_mesh), F(soc_terrain_layer, materials),
    F(soc_terrain_layer, material_count), F(soc_terrain_layer, shadow), F(soc_terrain_layer, visibility),
    F(soc_terrain_layer, workspace), F(soc_terrain_layer, shadow_workspace),
    F(soc_entity, position), F(soc_entity, rotation), F(soc_entity, scale), F(soc_entity, components),
    F(soc_entity, color), F(soc_entity, intensity), F(soc_entity, cut_off), F(soc_entity, outer_cut_off),
    F(soc_pass_desc, name), F(soc_pass_desc, group), F(soc_pass_desc, phase), F(soc_pass_desc, flags),
    F(soc_pass_desc, read_count), F(soc_pass_desc, write_count), F(soc_pass_desc, reads), F(soc_pass_desc, writes),
    F(soc_light_bounds, point_range), F(soc_light_bounds, spot_range),
    F(soc_sun_cascades, count), F(soc_sun_cascades, map_size), F(soc_sun_cascades, projection_view),
    F(soc_sun_cascades, split_depth), F(soc_sun_cascades, exponential_factor),
};
#undef F
struct TypeInfo { const char* type; size_t size; };
#define T(X) {#X, sizeof(X)}
const TypeInfo kTypes[] = {
    T(soc_img), T(soc_globals), T(soc_sun_info), T(soc_point_light), T(soc_spot_light), T(soc_auto_exposure), T(soc_camera),
    T(soc_frame_images), T(soc_mesh), T(soc_material), T(soc_raster_scene), T(soc_transform), T(soc_draw), T(soc_draw_scene),
    T(soc_terrain_layer), T(soc_pass_desc), T(soc_entity), T(soc_light_bounds), T(soc_sun_cascades),
};
#undef T
}  // namespace

extern "C" int32_t soc_abi_version(void) { return SOC_RT_ABI_VERSION; }

extern "C" size_t soc_abi_sizeof(const char* t) {
    for (const auto& e : kTypes)
        if (t && !std::strcmp(e.type, t)) return e.size;
    return 0;
}

extern "C" int64_t soc_abi_offsetof(const char* t, const char* f) {
    if (!t || !f) return -1;
    for (const auto& e : kFields)
        if (!std::strcmp(e.type, t) && !std::strcmp(e.field, f)) return (int64_t)e.offset;
    return -1;
}

extern "C" const char* soc_last_error_string(void) { return t_error.c_str(); }
extern "C" const char* soc_device_arch(void) { return "gfx950"; }

extern "C" void soc_tuning_reload(void) {
    std::lock_guard<std::mutex> lock(g_knob_mu);
    g_knobs.clear();
    g_knob_generation.fetch_add(1, std::memory_order_release);
}
