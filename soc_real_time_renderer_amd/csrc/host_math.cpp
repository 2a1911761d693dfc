// host_math.cpp — the globals feed: fp32 restatements of glm, the AgX matrices, the camera, the jitter and
// Scene::update (application.cpp, camera.cpp, renderer.cpp, scene.cpp of the reference).
//
// Compiled with -ffp-contract=off: this host fp32 math (AgX matrices, sun view-projection, glm restatements) performs
// exactly the roundings the oracle's C performs. It is the only host file that needs the flag.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstring>

#include "soc_internal.hpp"

namespace soc {

void mat4_mul_host(float out[16], const float a[16], const float b[16]) {
    float t[16];
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r)
            t[c * 4 + r] = a[0 * 4 + r] * b[c * 4 + 0] + a[1 * 4 + r] * b[c * 4 + 1] + a[2 * 4 + r] * b[c * 4 + 2] +
                           a[3 * 4 + r] * b[c * 4 + 3];
    std::memcpy(out, t, sizeof t);
}

// ---- AgX matrices (tone_mapping.inl:103-163), fp32, same operation order as the shader ----------
namespace {
struct H3 { float x, y, z; };
struct H2 { float x, y; };

void mat3_mul(float* out, const float* a, const float* b) {
    float t[9];
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) t[c * 3 + r] = a[0 * 3 + r] * b[c * 3 + 0] + a[1 * 3 + r] * b[c * 3 + 1] + a[2 * 3 + r] * b[c * 3 + 2];
    std::memcpy(out, t, sizeof t);
}
void mat3_inverse(float* o, const float* m) {
#define M(c, r) m[(c) * 3 + (r)]
    float det = M(0, 0) * (M(1, 1) * M(2, 2) - M(2, 1) * M(1, 2)) - M(1, 0) * (M(0, 1) * M(2, 2) - M(2, 1) * M(0, 2)) +
                M(2, 0) * (M(0, 1) * M(1, 2) - M(1, 1) * M(0, 2));
    float od = 1.0f / det;
    float t[9];
    t[0 * 3 + 0] = +(M(1, 1) * M(2, 2) - M(2, 1) * M(1, 2)) * od;
    t[1 * 3 + 0] = -(M(1, 0) * M(2, 2) - M(2, 0) * M(1, 2)) * od;
    t[2 * 3 + 0] = +(M(1, 0) * M(2, 1) - M(2, 0) * M(1, 1)) * od;
    t[0 * 3 + 1] = -(M(0, 1) * M(2, 2) - M(2, 1) * M(0, 2)) * od;
    t[1 * 3 + 1] = +(M(0, 0) * M(2, 2) - M(2, 0) * M(0, 2)) * od;
    t[2 * 3 + 1] = -(M(0, 0) * M(2, 1) - M(2, 0) * M(0, 1)) * od;
    t[0 * 3 + 2] = +(M(0, 1) * M(1, 2) - M(1, 1) * M(0, 2)) * od;
    t[1 * 3 + 2] = -(M(0, 0) * M(1, 2) - M(1, 0) * M(0, 2)) * od;
    t[2 * 3 + 2] = +(M(0, 0) * M(1, 1) - M(1, 0) * M(0, 1)) * od;
#undef M
    std::memcpy(o, t, sizeof t);
}
H3 unproject(H2 xy) {  // xyYToXYZ(vec3(xy, 1))
    float Y = 1.0f;
    float X = (xy.x * Y) / xy.y;
    float Z = ((1.0f - xy.x - xy.y) * Y) / xy.y;
    return H3{X, Y, Z};
}
void primaries_to_matrix(float* out, H2 r, H2 g, H2 b, H2 w) {
    H3 R = unproject(r), G = unproject(g), B = unproject(b), W = unproject(w);
    float temp[9] = {R.x, 1.0f, R.z, G.x, 1.0f, G.z, B.x, 1.0f, B.z};
    float it[9];
    mat3_inverse(it, temp);
    H3 s = H3{it[0] * W.x + it[3] * W.y + it[6] * W.z, it[1] * W.x + it[4] * W.y + it[7] * W.z,
              it[2] * W.x + it[5] * W.y + it[8] * W.z};
    float m[9] = {R.x * s.x, R.y * s.x, R.z * s.x, G.x * s.y, G.y * s.y, G.z * s.y, B.x * s.z, B.y * s.z, B.z * s.z};
    std::memcpy(out, m, sizeof m);
}
H2 mix2(H2 a, H2 b, float t) { return H2{a.x * (1.0f - t) + b.x * t, a.y * (1.0f - t) + b.y * t}; }
}  // namespace

void agx_matrices(float compression, float M[9], float Minv[9]) {
    const H2 xr{0.64f, 0.33f}, xg{0.3f, 0.6f}, xb{0.15f, 0.06f}, xw{0.3127f, 0.3290f};
    float srgb_to_xyz[9], adjusted_to_xyz[9], xyz_to_adjusted[9];
    primaries_to_matrix(srgb_to_xyz, xr, xg, xb, xw);
    const float sf = 1.0f / (1.0f - compression);
    primaries_to_matrix(adjusted_to_xyz, mix2(xw, xr, sf), mix2(xw, xg, sf), mix2(xw, xb, sf), xw);
    mat3_inverse(xyz_to_adjusted, adjusted_to_xyz);
    mat3_mul(M, srgb_to_xyz, xyz_to_adjusted);
    mat3_inverse(Minv, M);
}

}  // namespace soc

using namespace soc;

// =================================================================================================
// glm restatements (glm 0.9.9 / 1.0 scalar code paths, RH_NO clip control: quirk Q1)
// =================================================================================================
extern "C" void soc_mat4_mul(float out[16], const float a[16], const float b[16]) { mat4_mul_host(out, a, b); }

static inline void ident(float* m) {
    std::memset(m, 0, 16 * sizeof(float));
    m[0] = m[5] = m[10] = m[15] = 1.0f;
}

extern "C" void soc_mat4_perspective_rh_no(float out[16], float fovy, float aspect, float zNear, float zFar) {
    const float tanHalfFovy = std::tan(fovy / 2.0f);
    std::memset(out, 0, 16 * sizeof(float));
    out[0 * 4 + 0] = 1.0f / (aspect * tanHalfFovy);
    out[1 * 4 + 1] = 1.0f / tanHalfFovy;
    out[2 * 4 + 2] = -(zFar + zNear) / (zFar - zNear);
    out[2 * 4 + 3] = -1.0f;
    out[3 * 4 + 2] = -(2.0f * zFar * zNear) / (zFar - zNear);
}

extern "C" void soc_mat4_ortho_rh_no(float out[16], float l, float r, float b, float t, float zNear, float zFar) {
    ident(out);
    out[0 * 4 + 0] = 2.0f / (r - l);
    out[1 * 4 + 1] = 2.0f / (t - b);
    out[2 * 4 + 2] = -2.0f / (zFar - zNear);
    out[3 * 4 + 0] = -(r + l) / (r - l);
    out[3 * 4 + 1] = -(t + b) / (t - b);
    out[3 * 4 + 2] = -(zFar + zNear) / (zFar - zNear);
}

namespace {
struct V3h { float x, y, z; };
inline V3h sub(V3h a, V3h b) { return V3h{a.x - b.x, a.y - b.y, a.z - b.z}; }
inline float dot(V3h a, V3h b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V3h cross(V3h a, V3h b) { return V3h{a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }
inline V3h normalize(V3h v) {  // glm: v * inversesqrt(dot(v, v)), inversesqrt = 1 / sqrt
    float s = 1.0f / std::sqrt(dot(v, v));
    return V3h{v.x * s, v.y * s, v.z * s};
}
}  // namespace

extern "C" void soc_mat4_look_at_rh(float out[16], const float eye_[3], const float center_[3], const float up_[3]) {
    const V3h eye{eye_[0], eye_[1], eye_[2]}, center{center_[0], center_[1], center_[2]}, up{up_[0], up_[1], up_[2]};
    const V3h f = normalize(sub(center, eye));
    const V3h s = normalize(cross(f, up));
    const V3h u = cross(s, f);
    ident(out);
    out[0 * 4 + 0] = s.x; out[1 * 4 + 0] = s.y; out[2 * 4 + 0] = s.z;
    out[0 * 4 + 1] = u.x; out[1 * 4 + 1] = u.y; out[2 * 4 + 1] = u.z;
    out[0 * 4 + 2] = -f.x; out[1 * 4 + 2] = -f.y; out[2 * 4 + 2] = -f.z;
    out[3 * 4 + 0] = -dot(s, eye);
    out[3 * 4 + 1] = -dot(u, eye);
    out[3 * 4 + 2] = dot(f, eye);
}

// glm compute_inverse<4,4> (func_matrix.inl), scalar path.
extern "C" void soc_mat4_inverse(float out[16], const float mm[16]) {
#define m(c, r) mm[(c) * 4 + (r)]
    const float Coef00 = m(2, 2) * m(3, 3) - m(3, 2) * m(2, 3);
    const float Coef02 = m(1, 2) * m(3, 3) - m(3, 2) * m(1, 3);
    const float Coef03 = m(1, 2) * m(2, 3) - m(2, 2) * m(1, 3);
    const float Coef04 = m(2, 1) * m(3, 3) - m(3, 1) * m(2, 3);
    const float Coef06 = m(1, 1) * m(3, 3) - m(3, 1) * m(1, 3);
    const float Coef07 = m(1, 1) * m(2, 3) - m(2, 1) * m(1, 3);
    const float Coef08 = m(2, 1) * m(3, 2) - m(3, 1) * m(2, 2);
    const float Coef10 = m(1, 1) * m(3, 2) - m(3, 1) * m(1, 2);
    const float Coef11 = m(1, 1) * m(2, 2) - m(2, 1) * m(1, 2);
    const float Coef12 = m(2, 0) * m(3, 3) - m(3, 0) * m(2, 3);
    const float Coef14 = m(1, 0) * m(3, 3) - m(3, 0) * m(1, 3);
    const float Coef15 = m(1, 0) * m(2, 3) - m(2, 0) * m(1, 3);
    const float Coef16 = m(2, 0) * m(3, 2) - m(3, 0) * m(2, 2);
    const float Coef18 = m(1, 0) * m(3, 2) - m(3, 0) * m(1, 2);
    const float Coef19 = m(1, 0) * m(2, 2) - m(2, 0) * m(1, 2);
    const float Coef20 = m(2, 0) * m(3, 1) - m(3, 0) * m(2, 1);
    const float Coef22 = m(1, 0) * m(3, 1) - m(3, 0) * m(1, 1);
    const float Coef23 = m(1, 0) * m(2, 1) - m(2, 0) * m(1, 1);
    const float Fac0[4] = {Coef00, Coef00, Coef02, Coef03};
    const float Fac1[4] = {Coef04, Coef04, Coef06, Coef07};
    const float Fac2[4] = {Coef08, Coef08, Coef10, Coef11};
    const float Fac3[4] = {Coef12, Coef12, Coef14, Coef15};
    const float Fac4[4] = {Coef16, Coef16, Coef18, Coef19};
    const float Fac5[4] = {Coef20, Coef20, Coef22, Coef23};
    const float Vec0[4] = {m(1, 0), m(0, 0), m(0, 0), m(0, 0)};
    const float Vec1[4] = {m(1, 1), m(0, 1), m(0, 1), m(0, 1)};
    const float Vec2[4] = {m(1, 2), m(0, 2), m(0, 2), m(0, 2)};
    const float Vec3[4] = {m(1, 3), m(0, 3), m(0, 3), m(0, 3)};
    float Inv[4][4];
    for (int i = 0; i < 4; ++i) {
        Inv[0][i] = Vec1[i] * Fac0[i] - Vec2[i] * Fac1[i] + Vec3[i] * Fac2[i];
        Inv[1][i] = Vec0[i] * Fac0[i] - Vec2[i] * Fac3[i] + Vec3[i] * Fac4[i];
        Inv[2][i] = Vec0[i] * Fac1[i] - Vec1[i] * Fac3[i] + Vec3[i] * Fac5[i];
        Inv[3][i] = Vec0[i] * Fac2[i] - Vec1[i] * Fac4[i] + Vec2[i] * Fac5[i];
    }
    const float SignA[4] = {+1.0f, -1.0f, +1.0f, -1.0f}, SignB[4] = {-1.0f, +1.0f, -1.0f, +1.0f};
    float Inverse[4][4];
    for (int i = 0; i < 4; ++i) {
        Inverse[0][i] = Inv[0][i] * SignA[i];
        Inverse[1][i] = Inv[1][i] * SignB[i];
        Inverse[2][i] = Inv[2][i] * SignA[i];
        Inverse[3][i] = Inv[3][i] * SignB[i];
    }
    const float Row0[4] = {Inverse[0][0], Inverse[1][0], Inverse[2][0], Inverse[3][0]};
    const float Dot0[4] = {m(0, 0) * Row0[0], m(0, 1) * Row0[1], m(0, 2) * Row0[2], m(0, 3) * Row0[3]};
    const float Dot1 = (Dot0[0] + Dot0[1]) + (Dot0[2] + Dot0[3]);
    const float OneOverDeterminant = 1.0f / Dot1;
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) out[c * 4 + r] = Inverse[c][r] * OneOverDeterminant;
#undef m
}

static inline float radians(float deg) { return deg * 0.01745329251994329576923690768489f; }

// glm::rotateX/Y/Z (gtx/rotate_vector.inl)
static V3h rotate_x(V3h v, float a) { float c = std::cos(a), s = std::sin(a); return V3h{v.x, v.y * c - v.z * s, v.y * s + v.z * c}; }
static V3h rotate_y(V3h v, float a) { float c = std::cos(a), s = std::sin(a); return V3h{v.x * c + v.z * s, v.y, -v.x * s + v.z * c}; }
static V3h rotate_z(V3h v, float a) { float c = std::cos(a), s = std::sin(a); return V3h{v.x * c - v.y * s, v.x * s + v.y * c, v.z}; }

extern "C" int soc_globals_init_defaults(soc_globals* g, int32_t width, int32_t height) {
    if (!g || width <= 0 || height <= 0) return set_error(SOC_E_INVALID_ARG, "soc_globals_init_defaults: bad args");
    std::memset(g, 0, sizeof *g);
    // renderer.cpp:72-107
    g->terrain_offset[0] = g->terrain_offset[1] = g->terrain_offset[2] = 0.0f;
    g->terrain_scale[0] = g->terrain_scale[1] = 100.0f;
    g->terrain_height_scale = 70.0f;
    g->terrain_midpoint = 0.2f;
    g->terrain_delta = 8.0f;
    g->terrain_min_depth = 1.0f;
    g->terrain_max_depth = 100.0f;
    g->terrain_min_tess_level = 1;
    g->terrain_max_tess_level = 3;
    g->ssao_bias = 0.025f;
    g->ssao_radius = 0.3f;
    g->ssao_kernel_size = 26;
    g->ambient[0] = g->ambient[1] = g->ambient[2] = 0.1f;
    g->ambient_occlussion_strength = 1.2f;
    g->emissive_bloom_strength = 2.0f;
    g->focal_length = 5.0f;
    g->plane_in_focus = 1.0f;
    g->aperture = 8.0f;
    g->adjustment_speed = 1.0f;
    g->log_min_luminance = -15.0f;
    g->log_max_luminance = 15.0f;
    g->target_luminance = 0.2140f;
    g->elapsed_time = 0.0f;
    g->log_min_luminance = std::log2(g->target_luminance / std::exp2(g->log_min_luminance));
    g->log_max_luminance = std::log2(g->target_luminance / std::exp2(g->log_max_luminance));
    g->saturation = 1.0f;
    g->agxDs_linear_section = 0.18f;
    g->peak = 1.0f;
    g->compression = 0.15f;
    g->frame_counter = 0;
    // sun, renderer.cpp:109-133 (angle_direction = {4, 0, 0}, renderer.hpp:67)
    const V3h light_position{-3.2f, 40.0f, -4.0f};
    const float planes = 16.0f;
    float light_projection[16];
    soc_mat4_ortho_rh_no(light_projection, -planes, planes, -planes, planes, -planes, planes);
    V3h dir{0.0f, -1.0f, 0.0f};
    dir = rotate_x(dir, radians(4.0f));
    dir = rotate_y(dir, radians(0.0f));
    dir = rotate_z(dir, radians(0.0f));
    const float eye[3] = {light_position.x, light_position.y, light_position.z};
    const float center[3] = {light_position.x + dir.x, light_position.y + dir.y, light_position.z + dir.z};
    const float up[3] = {0.0f, -1.0f, 0.0f};
    float light_view[16], pv[16];
    soc_mat4_look_at_rh(light_view, eye, center, up);
    mat4_mul_host(pv, light_projection, light_view);
    std::memcpy(g->sun_info.projection_matrix, light_projection, sizeof light_projection);
    std::memcpy(g->sun_info.view_matrix, light_view, sizeof light_view);
    std::memcpy(g->sun_info.projection_view_matrix, pv, sizeof pv);
    for (int r = 0; r < 4; ++r) g->sun_info.terrain_y_clip_trick[r] = pv[1 * 4 + r];  // pv * (0,1,0,0)
    g->sun_info.position[0] = light_position.x; g->sun_info.position[1] = light_position.y; g->sun_info.position[2] = light_position.z;
    g->sun_info.direction[0] = dir.x; g->sun_info.direction[1] = dir.y; g->sun_info.direction[2] = dir.z;
    g->sun_info.exponential_factor = -80.0f;
    g->sun_info.darkening_factor = 1.0f;
    g->sun_info.bias = 0.0001f;
    g->sun_info.intensity = 1.0f;
    g->resolution[0] = width;
    g->resolution[1] = height;
    // Camera3D defaults (camera.hpp:74-75)
    g->camera_near_clip = 0.1f;
    g->camera_far_clip = 1000.0f;
    return SOC_OK;
}

extern "C" int soc_globals_frame_update(soc_globals* g, const soc_camera* cam, int32_t width, int32_t height, float delta_time,
                                        uint32_t* jitter_index) {
    if (!g || !cam || !jitter_index || width <= 0 || height <= 0)
        return set_error(SOC_E_INVALID_ARG, "soc_globals_frame_update: bad args");
    // Camera3D::resize (camera.cpp:6-10)
    float proj[16];
    const float aspect = (float)width / (float)height;
    soc_mat4_perspective_rh_no(proj, radians(cam->fov_degrees), aspect, cam->near_clip, cam->far_clip);
    proj[1 * 4 + 1] *= -1.0f;
    // ControlledCamera3D::update (camera.cpp:36-56), no input
    float ry = cam->rotation[1];
    const float MAX_ROT = 1.56825555556f;
    if (ry > MAX_ROT) ry = MAX_ROT;
    if (ry < -MAX_ROT) ry = -MAX_ROT;
    const float rx = cam->rotation[0];
    const V3h fwd = normalize(V3h{std::cos(rx) * std::cos(ry), -std::sin(ry), std::sin(rx) * std::cos(ry)});
    const float eye[3] = {cam->position[0], cam->position[1], cam->position[2]};
    const float center[3] = {eye[0] + fwd.x, eye[1] + fwd.y, eye[2] + fwd.z};
    const float up[3] = {0.0f, 1.0f, 0.0f};
    float view[16];
    soc_mat4_look_at_rh(view, eye, center, up);
    // Application::update jitter (application.cpp:113-131)
    const float gr = 1.32471795724474602596f, a1 = 1.0f / gr, a2 = 1.0f / (gr * gr);
    auto gmod = [](float x, float y) { return x - y * std::floor(x / y); };
    const float idx = (float)(*jitter_index);
    float jx = gmod(0.5f + a1 * (idx + 1.0f), 1.0f) - 0.5f;
    float jy = gmod(0.5f + a2 * (idx + 1.0f), 1.0f) - 0.5f;
    jx = jx * (1.0f / (float)width);
    jy = jy * (1.0f / (float)height);
    *jitter_index = (*jitter_index + 1) % 32;
    proj[3 * 4 + 0] += jx;
    proj[3 * 4 + 1] += jy;
    float inv_proj[16], inv_view[16], pv[16], inv_pv[16];
    soc_mat4_inverse(inv_proj, proj);
    soc_mat4_inverse(inv_view, view);
    mat4_mul_host(pv, proj, view);
    mat4_mul_host(inv_pv, inv_proj, inv_view);
    // shift current -> previous (application.cpp:139-146)
    std::memcpy(g->camera_previous_projection_matrix, g->camera_projection_matrix, 64);
    std::memcpy(g->camera_previous_inverse_projection_matrix, g->camera_inverse_projection_matrix, 64);
    std::memcpy(g->camera_previous_view_matrix, g->camera_view_matrix, 64);
    std::memcpy(g->camera_previous_inverse_view_matrix, g->camera_inverse_view_matrix, 64);
    std::memcpy(g->camera_previous_projection_view_matrix, g->camera_projection_view_matrix, 64);
    std::memcpy(g->camera_previous_inverse_projection_view_matrix, g->camera_inverse_projection_view_matrix, 64);
    std::memcpy(g->terrain_previous_y_clip_trick, g->terrain_y_clip_trick, 16);
    std::memcpy(g->previous_jitter, g->jitter, 8);
    std::memcpy(g->camera_projection_matrix, proj, 64);
    std::memcpy(g->camera_inverse_projection_matrix, inv_proj, 64);
    std::memcpy(g->camera_view_matrix, view, 64);
    std::memcpy(g->camera_inverse_view_matrix, inv_view, 64);
    std::memcpy(g->camera_projection_view_matrix, pv, 64);
    std::memcpy(g->camera_inverse_projection_view_matrix, inv_pv, 64);
    for (int r = 0; r < 4; ++r) g->terrain_y_clip_trick[r] = pv[1 * 4 + r];
    g->jitter[0] = jx;
    g->jitter[1] = jy;
    g->camera_near_clip = cam->near_clip;
    g->camera_far_clip = cam->far_clip;
    g->resolution[0] = width;
    g->resolution[1] = height;
    for (int i = 0; i < 3; ++i) g->camera_position[i] = cam->position[i];
    g->delta_time = delta_time;
    g->elapsed_time += delta_time;
    g->frame_counter++;
    return SOC_OK;
}

// Scene::update (src/ecs/scene.cpp:47-118): transforms (glm translate * toMat4(quat(euler)) * scale, and
// transpose(inverse(model))) and the light lists.
static void quat_euler_to_mat4(float out[16], const float euler_rad[3]) {
    // glm::qua(vec3 eulerAngle) (gtc/quaternion.inl) then mat3_cast / toMat4 (gtx/quaternion.inl)
    const float cx = std::cos(euler_rad[0] * 0.5f), cy = std::cos(euler_rad[1] * 0.5f), cz = std::cos(euler_rad[2] * 0.5f);
    const float sx = std::sin(euler_rad[0] * 0.5f), sy = std::sin(euler_rad[1] * 0.5f), sz = std::sin(euler_rad[2] * 0.5f);
    const float w = cx * cy * cz + sx * sy * sz;
    const float x = sx * cy * cz - cx * sy * sz;
    const float y = cx * sy * cz + sx * cy * sz;
    const float z = cx * cy * sz - sx * sy * cz;
    const float qxx = x * x, qyy = y * y, qzz = z * z, qxz = x * z, qxy = x * y, qyz = y * z, qwx = w * x, qwy = w * y,
                qwz = w * z;
    ident(out);
    out[0 * 4 + 0] = 1.0f - 2.0f * (qyy + qzz);
    out[0 * 4 + 1] = 2.0f * (qxy + qwz);
    out[0 * 4 + 2] = 2.0f * (qxz - qwy);
    out[1 * 4 + 0] = 2.0f * (qxy - qwz);
    out[1 * 4 + 1] = 1.0f - 2.0f * (qxx + qzz);
    out[1 * 4 + 2] = 2.0f * (qyz + qwx);
    out[2 * 4 + 0] = 2.0f * (qxz + qwy);
    out[2 * 4 + 1] = 2.0f * (qyz - qwx);
    out[2 * 4 + 2] = 1.0f - 2.0f * (qxx + qyy);
}

extern "C" int soc_scene_update(soc_globals* g, const soc_entity* e, int32_t count, float* model_matrices,
                                float* normal_matrices) {
    if (!g || count < 0 || (count > 0 && !e)) return set_error(SOC_E_INVALID_ARG, "soc_scene_update: bad arguments");
    int np = 0, ns = 0;
    for (int i = 0; i < count; ++i) {
        np += (e[i].components & SOC_ENTITY_POINT_LIGHT) ? 1 : 0;
        ns += (e[i].components & SOC_ENTITY_SPOT_LIGHT) ? 1 : 0;
    }
    if (np > SOC_MAX_POINT_LIGHTS || ns > SOC_MAX_SPOT_LIGHTS)
        return set_error(SOC_E_SHAPE, "soc_scene_update: %d point / %d spot lights exceed %d / %d", np, ns,
                         SOC_MAX_POINT_LIGHTS, SOC_MAX_SPOT_LIGHTS);
    g->point_light_count = 0;
    g->spot_light_count = 0;
    for (int i = 0; i < count; ++i) {
        const soc_entity& t = e[i];
        if (model_matrices || normal_matrices) {   // scene.cpp:64-68
            float T[16], R[16], S[16], TR[16], M[16], inv[16];
            ident(T);
            T[12] = t.position[0];
            T[13] = t.position[1];
            T[14] = t.position[2];
            const float eul[3] = {radians(t.rotation[0]), radians(t.rotation[1]), radians(t.rotation[2])};
            quat_euler_to_mat4(R, eul);
            ident(S);
            S[0] = t.scale[0];
            S[5] = t.scale[1];
            S[10] = t.scale[2];
            mat4_mul_host(TR, T, R);
            mat4_mul_host(M, TR, S);
            if (model_matrices) std::memcpy(model_matrices + 16 * i, M, sizeof M);
            if (normal_matrices) {
                soc_mat4_inverse(inv, M);
                for (int c = 0; c < 4; ++c)
                    for (int r = 0; r < 4; ++r) normal_matrices[16 * i + c * 4 + r] = inv[r * 4 + c];
            }
        }
        if (t.components & SOC_ENTITY_POINT_LIGHT) {   // scene.cpp:87-96
            soc_point_light& L = g->point_lights[g->point_light_count++];
            for (int k = 0; k < 3; ++k) {
                L.position[k] = t.position[k];
                L.color[k] = t.color[k];
            }
            L.intensity = t.intensity;
        }
        if (t.components & SOC_ENTITY_SPOT_LIGHT) {    // scene.cpp:98-116
            V3h dir{0.0f, -1.0f, 0.0f};
            dir = rotate_x(dir, radians(t.rotation[0]));
            dir = rotate_y(dir, radians(t.rotation[1]));
            dir = rotate_z(dir, radians(t.rotation[2]));
            soc_spot_light& L = g->spot_lights[g->spot_light_count++];
            for (int k = 0; k < 3; ++k) {
                L.position[k] = t.position[k];
                L.color[k] = t.color[k];
            }
            L.direction[0] = dir.x;
            L.direction[1] = dir.y;
            L.direction[2] = dir.z;
            L.intensity = t.intensity;
            L.cut_off = std::cos(radians(t.cut_off));
            L.outer_cut_off = std::cos(radians(t.outer_cut_off));
        }
    }
    return SOC_OK;
}

extern "C" int soc_upload_globals(const soc_globals* g, soc_globals* d_globals, soc_stream stream) {
    if (!g || !d_globals) return set_error(SOC_E_INVALID_ARG, "soc_upload_globals: null argument");
    hipError_t e = hipMemcpyAsync(d_globals, g, sizeof(soc_globals), hipMemcpyHostToDevice, hs(stream));
    if (e != hipSuccess) return set_error(SOC_E_HIP, "soc_upload_globals: %s", hipGetErrorString(e));
    return SOC_OK;
}

// The device record of the light ranges (LightBoundsDev): validated first, converted on the host, one copy.
extern "C" int soc_upload_light_bounds(const soc_light_bounds* host, void* d_bounds, soc_stream stream) {
    if (!host || !d_bounds) return set_error(SOC_E_INVALID_ARG, "soc_upload_light_bounds: null argument");
    LightBoundsDev rec;
    auto convert = [](const float* range, int n, const char* kind, float* inv_r2, float* r2) {
        for (int i = 0; i < n; ++i) {
            const float r = range[i];
            if (!(r >= 0.0f) || std::isinf(r))
                return set_error(SOC_E_INVALID_ARG, "soc_upload_light_bounds: %s_range[%d] = %g (0 or a finite range > 0)", kind,
                                 i, (double)r);
            if (r == 0.0f) {
                inv_r2[i] = r2[i] = 0.0f;
                continue;
            }
            // r * r over fp32: unlimited to every fp32 distance; under it: the smallest normal square
            float q = r * r;
            if (std::isinf(q)) {
                inv_r2[i] = r2[i] = 0.0f;
                continue;
            }
            if (q < FLT_MIN) q = FLT_MIN;
            const float inv = 1.0f / q;
            if (inv < FLT_MIN) {   // the window would be 1 to within fp32 everywhere a distance is finite
                inv_r2[i] = r2[i] = 0.0f;
                continue;
            }
            inv_r2[i] = inv;
            r2[i] = q;
        }
        return (int)SOC_OK;
    };
    int rc = convert(host->point_range, SOC_MAX_POINT_LIGHTS, "point", rec.point_inv_r2, rec.point_r2);
    if (!rc) rc = convert(host->spot_range, SOC_MAX_SPOT_LIGHTS, "spot", rec.spot_inv_r2, rec.spot_r2);
    if (rc) return rc;
    // pageable source: the copy is staged before hipMemcpyAsync returns, so `rec` may leave scope
    hipError_t e = hipMemcpyAsync(d_bounds, &rec, sizeof rec, hipMemcpyHostToDevice, hs(stream));
    if (e != hipSuccess) return set_error(SOC_E_HIP, "soc_upload_light_bounds: %s", hipGetErrorString(e));
    return SOC_OK;
}

// =================================================================================================
// Cascaded sun shadow maps (soc_rt.h): the record's validation and the fit. Host fp32, no HIP call.
// =================================================================================================
int soc::check_sun_cascades(const soc_sun_cascades* c, const soc_img* atlas, const char* P) {
    if (!c) return set_error(SOC_E_INVALID_ARG, "%s: null cascades", P);
    if (c->count < 1 || c->count > SOC_MAX_SUN_CASCADES)
        return set_error(SOC_E_INVALID_ARG, "%s: cascades count = %d (1..%d)", P, c->count, SOC_MAX_SUN_CASCADES);
    if (c->map_size < 2) return set_error(SOC_E_INVALID_ARG, "%s: cascades map_size = %d (>= 2)", P, c->map_size);
    if (c->map_size > 16384) return set_error(SOC_E_INVALID_ARG, "%s: cascades map_size = %d (<= 16384)", P, c->map_size);
    for (int k = 0; k < c->count; ++k) {
        for (int i = 0; i < 16; ++i)
            if (!std::isfinite(c->projection_view[k][i]))
                return set_error(SOC_E_INVALID_ARG, "%s: cascades projection_view[%d][%d] is not finite", P, k, i);
        if (!std::isfinite(c->exponential_factor[k]))
            return set_error(SOC_E_INVALID_ARG, "%s: cascades exponential_factor[%d] is not finite", P, k);
    }
    for (int i = 0; i + 1 < c->count; ++i) {
        if (!std::isfinite(c->split_depth[i]))
            return set_error(SOC_E_INVALID_ARG, "%s: cascades split_depth[%d] is not finite", P, i);
        if (i > 0 && !(c->split_depth[i] > c->split_depth[i - 1]))
            return set_error(SOC_E_INVALID_ARG, "%s: cascades split_depth[%d] = %g is not above split_depth[%d] = %g", P, i,
                             (double)c->split_depth[i], i - 1, (double)c->split_depth[i - 1]);
    }
    if (atlas) {
        if (atlas->format != SOC_FMT_D32F)
            return set_error(SOC_E_INVALID_ARG, "%s: cascades atlas format %d is not D32F", P, atlas->format);
        if (atlas->width != c->map_size || (int64_t)atlas->height != (int64_t)c->count * c->map_size)
            return set_error(SOC_E_INVALID_ARG, "%s: cascades atlas extent %dx%d is not map_size x count*map_size = %dx%d", P,
                             atlas->width, atlas->height, c->map_size, c->count * c->map_size);
    }
    return SOC_OK;
}

extern "C" int soc_sun_cascades_from_sun(const soc_globals* g, int32_t map_size, soc_sun_cascades* out) {
    static const char* P = "soc_sun_cascades_from_sun";
    if (!g || !out) return set_error(SOC_E_INVALID_ARG, "%s: null argument", P);
    if (map_size < 2) return set_error(SOC_E_INVALID_ARG, "%s: map_size = %d (>= 2)", P, map_size);
    soc_sun_cascades c;
    std::memset(&c, 0, sizeof c);
    c.count = 1;
    c.map_size = map_size;
    mat4_mul_host(c.projection_view[0], g->sun_info.projection_matrix, g->sun_info.view_matrix);
    c.exponential_factor[0] = g->sun_info.exponential_factor;
    const int rc = check_sun_cascades(&c, nullptr, P);
    if (rc) return rc;
    *out = c;
    return SOC_OK;
}

// The radius quantum of a cascade's bounding sphere (world units): the orthographic extent only takes multiples of it.
static const float kCascadeRadiusQuantum = 0.125f;

extern "C" int soc_sun_cascades_fit(const soc_globals* g, int32_t count, int32_t map_size, float near_distance,
                                    float max_distance, float split_lambda, float caster_margin, soc_sun_cascades* out) {
    static const char* P = "soc_sun_cascades_fit";
    if (!g || !out) return set_error(SOC_E_INVALID_ARG, "%s: null argument", P);
    if (count < 1 || count > SOC_MAX_SUN_CASCADES)
        return set_error(SOC_E_INVALID_ARG, "%s: count = %d (1..%d)", P, count, SOC_MAX_SUN_CASCADES);
    if (map_size < 2 || map_size > 16384) return set_error(SOC_E_INVALID_ARG, "%s: map_size = %d (2..16384)", P, map_size);
    if (!std::isfinite(near_distance) || !std::isfinite(max_distance) || !(near_distance > 0.0f) || !(max_distance > near_distance))
        return set_error(SOC_E_INVALID_ARG, "%s: near_distance = %g, max_distance = %g (0 < near < max, finite)", P,
                         (double)near_distance, (double)max_distance);
    if (!(split_lambda >= 0.0f && split_lambda <= 1.0f))
        return set_error(SOC_E_INVALID_ARG, "%s: split_lambda = %g (0..1)", P, (double)split_lambda);
    if (!(caster_margin >= 0.0f) || !std::isfinite(caster_margin))
        return set_error(SOC_E_INVALID_ARG, "%s: caster_margin = %g (finite, >= 0)", P, (double)caster_margin);
    // the camera's projection without the frame's jitter (application.cpp:113-131 adds it to proj[3][0..1])
    float pj[16];
    std::memcpy(pj, g->camera_projection_matrix, sizeof pj);
    pj[12] -= g->jitter[0];
    pj[13] -= g->jitter[1];
    if (pj[0] == 0.0f || pj[5] == 0.0f) return set_error(SOC_E_INVALID_ARG, "%s: the globals hold no camera projection", P);
    soc_sun_cascades c;
    std::memset(&c, 0, sizeof c);
    c.count = count;
    c.map_size = map_size;
    // slice distances
    float dist[SOC_MAX_SUN_CASCADES + 1];
    dist[0] = near_distance;
    const float n = near_distance, f = max_distance, N = (float)count;
    for (int i = 1; i <= count; ++i) {
        const float t = (float)i / N;
        dist[i] = i == count ? f : split_lambda * (n * std::pow(f / n, t)) + (1.0f - split_lambda) * (n + (f - n) * t);
    }
    for (int i = 0; i + 1 < count; ++i) {   // the depth-buffer value of (0, 0, -d, 1): z only
        const float z = -dist[i + 1];
        c.split_depth[i] = (pj[10] * z + pj[14]) / (pj[11] * z + pj[15]);
    }
    // the light's rotation: lookAt from the origin along the sun's direction, the reference's up (renderer.cpp:126)
    const float zero[3] = {0.0f, 0.0f, 0.0f}, up[3] = {0.0f, -1.0f, 0.0f};
    float rot[16];
    soc_mat4_look_at_rh(rot, zero, g->sun_info.direction, up);
    rot[12] = rot[13] = rot[14] = 0.0f;   // -dot(s, 0): -0
    const float S = (float)map_size;
    for (int k = 0; k < count; ++k) {
        // the slice's eight corners in view space, their centroid and the bounding sphere around it: all of it depends
        // on the projection and the distances only, so neither a rotation nor a translation of the camera changes it
        V3h corner[8];
        V3h mid{0.0f, 0.0f, 0.0f};
        for (int j = 0; j < 8; ++j) {
            const float z = -dist[k + (j >> 2)];
            const float w = pj[11] * z + pj[15];
            const float sx = (j & 1) ? 1.0f : -1.0f, sy = (j & 2) ? 1.0f : -1.0f;
            corner[j] = V3h{(sx * w - pj[8] * z - pj[12]) / pj[0], (sy * w - pj[9] * z - pj[13]) / pj[5], z};
            mid = V3h{mid.x + corner[j].x, mid.y + corner[j].y, mid.z + corner[j].z};
        }
        mid = V3h{mid.x * 0.125f, mid.y * 0.125f, mid.z * 0.125f};
        float r2 = 0.0f;
        for (int j = 0; j < 8; ++j) {
            const V3h d = sub(corner[j], mid);
            r2 = std::fmax(r2, dot(d, d));
        }
        // room for the snap (at most half a texel = R / S per axis) and for fp32, then up to the quantum
        const float need = std::sqrt(r2) / (1.0f - 1.0f / S) * 1.00001f;
        const float R = std::ceil(need / kCascadeRadiusQuantum) * kCascadeRadiusQuantum;
        const float D = 2.0f * R + caster_margin;   // the depth range that lands in z_ndc [0, 1] (quirk Q1: the raster keeps that half)
        float proj[16];
        soc_mat4_ortho_rh_no(proj, -R, R, -R, R, -D, D);
        // the centre in world and in light space; x and y snapped to whole texels, z so that the sphere and caster_margin
        // towards the sun sit in view z [-D, 0]
        const float* iv = g->camera_inverse_view_matrix;
        const V3h cw{iv[0] * mid.x + iv[4] * mid.y + iv[8] * mid.z + iv[12], iv[1] * mid.x + iv[5] * mid.y + iv[9] * mid.z + iv[13],
                     iv[2] * mid.x + iv[6] * mid.y + iv[10] * mid.z + iv[14]};
        const V3h cl{rot[0] * cw.x + rot[4] * cw.y + rot[8] * cw.z, rot[1] * cw.x + rot[5] * cw.y + rot[9] * cw.z,
                     rot[2] * cw.x + rot[6] * cw.y + rot[10] * cw.z};
        const float texel = (2.0f * R) / S;
        float view[16];
        std::memcpy(view, rot, sizeof view);
        view[12] = -(std::floor(cl.x / texel + 0.5f) * texel);
        view[13] = -(std::floor(cl.y / texel + 0.5f) * texel);
        view[14] = -(R + caster_margin) - cl.z;
        mat4_mul_host(c.projection_view[k], proj, view);
        c.exponential_factor[k] = g->sun_info.exponential_factor * g->sun_info.projection_matrix[10] / proj[10];
    }
    const int rc = check_sun_cascades(&c, nullptr, P);
    if (rc) return rc;
    *out = c;
    return SOC_OK;
}
