// san_host — drives the host code under AddressSanitizer + UndefinedBehaviorSanitizer (tools/sanitize/Makefile).
// No GPU call is made: the globals feed and ECS scene feed, ABI introspection, the render graph (construction,
// caller passes, derived and ring dependencies, raster head, error paths), the clouds, Composition, TAA, SSAO and bloom planners, the raster workspaces and
// the draw scenes' host checks, the PNG / EXR writers, the scene synthesiser, and every pass of the CPU oracle on small
// images (odd extents included). Exit 0 when every check passes; a sanitizer report aborts the run
// (-fno-sanitize-recover).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "soc_oracle.h"
#include "soc_rt.h"

extern "C" {
int soc_scene_gbuffer(int scene_id, const soc_globals* g, int W, int H, uint16_t* albedo, uint16_t* emissive,
                      uint16_t* normal, float* depth, uint16_t* velocity);
int soc_scene_shadow(int scene_id, const soc_globals* g, int S, float* shadow);
int soc_scene_mesh_counts(int scene_id, int* vertices, int* triangles);
int soc_scene_mesh(int scene_id, const soc_globals* g, float* positions, float* normals, float* uvs, uint32_t* indices,
                   uint32_t* materials);
int soc_scene_material_count(int scene_id);
int soc_scene_material_textures(int scene_id, const soc_globals* g, int size, uint8_t* rgba, float* emissive_rgb);
int soc_scene_terrain_heightmap(int size, uint8_t* rgba);
// test hook of the frame planner (csrc/render_execute.cpp), not in the public header
int64_t soc_debug_plan_frame(soc_renderer* r, const soc_globals* g, int32_t phase, int32_t sky_lane_high, int32_t advance,
                             char* buf, size_t cap);
// test hooks of the clouds planner (csrc/clouds_plan.cpp), not in the public header
int64_t soc_debug_plan_clouds(const soc_globals* g, soc_img depth, soc_img noise, soc_img target, void* workspace,
                              int32_t sky_bound, const int32_t residency[6], void* state, char* buf, size_t cap);
size_t soc_debug_cloud_state_bytes(void);
// test hook of the Composition planner (csrc/composition_plan.cpp), not in the public header
int64_t soc_debug_plan_composition(const soc_globals* g, const soc_globals* d_globals, const soc_img* images, uint32_t what,
                                   soc_auto_exposure* ae, uint32_t* scratch, const soc_img* mip1, const soc_img* mip3,
                                   const void* d_bounds, uint32_t light_flags, uint32_t* d_shaded,
                                   const soc_sun_cascades* cascades, char* buf, size_t cap);
// test hook of the TAA, SSAO and bloom planners (csrc/post_plan.cpp), not in the public header
int64_t soc_debug_plan_post(int32_t pass, const soc_globals* g, const soc_img* images, int32_t n_images, const void* aux,
                            int32_t arg, const int32_t* resident, char* buf, size_t cap);
}

namespace {
int g_fail = 0;
void expect(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "FAILED: %s (%s)\n", what, soc_last_error_string());
        ++g_fail;
    }
}

struct HostImg {
    std::vector<uint8_t> data;
    soc_img img;
    HostImg(int w, int h, int fmt, int bpp, uint8_t fill = 0) : data((size_t)w * h * bpp, fill) {
        img = soc_img{data.data(), w, h, w * bpp, fmt};
    }
};

uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

void fill_rgba16f(HostImg& im, uint32_t seed, float lo, float hi) {
    uint16_t* p = reinterpret_cast<uint16_t*>(im.data.data());
    for (size_t i = 0; i < im.data.size() / 2; ++i)
        p[i] = soc_oracle_f32_to_f16(lo + (hi - lo) * (float)(lcg(seed) >> 8) / 16777216.0f);
}

int32_t count_pass(void* user, const soc_globals*, const soc_frame_images*, soc_stream) {
    ++*static_cast<int*>(user);
    return 0;
}

void globals_and_scene_feed(soc_globals& g, int W, int H) {
    expect(soc_globals_init_defaults(&g, W, H) == SOC_OK, "soc_globals_init_defaults");
    soc_camera cam{{-14.0f, 2.2f, 0.3f}, {0.0f, -0.42f, 0.0f}, 90.0f, 0.1f, 1000.0f};
    uint32_t ji = 0;
    for (int i = 0; i < 3; ++i) {
        expect(soc_globals_frame_update(&g, &cam, W, H, 0.016f, &ji) == SOC_OK, "soc_globals_frame_update");
        cam.position[0] += 0.05f;
    }
    std::vector<soc_entity> ents(SOC_MAX_POINT_LIGHTS + SOC_MAX_SPOT_LIGHTS);
    for (size_t i = 0; i < ents.size(); ++i) {
        soc_entity& e = ents[i];
        std::memset(&e, 0, sizeof e);
        e.position[0] = -10.0f + 0.1f * (float)i;
        e.position[1] = 2.0f;
        e.scale[0] = e.scale[1] = e.scale[2] = 1.0f;
        e.rotation[0] = 5.0f * (float)i;
        e.components = i < SOC_MAX_POINT_LIGHTS ? SOC_ENTITY_POINT_LIGHT : SOC_ENTITY_SPOT_LIGHT;
        e.color[0] = e.color[1] = e.color[2] = 0.8f;
        e.intensity = 2.0f;
        e.cut_off = 12.5f;
        e.outer_cut_off = 17.5f;
    }
    std::vector<float> models(ents.size() * 16), normals(ents.size() * 16);
    expect(soc_scene_update(&g, ents.data(), (int)ents.size(), models.data(), normals.data()) == SOC_OK, "soc_scene_update");
    expect(g.point_light_count == SOC_MAX_POINT_LIGHTS && g.spot_light_count == SOC_MAX_SPOT_LIGHTS, "light counts");
    ents.push_back(ents.front());   // one light too many: an error, no write past the arrays
    expect(soc_scene_update(&g, ents.data(), (int)ents.size(), nullptr, nullptr) != SOC_OK, "light overflow rejected");
    float m[16], inv[16];
    const float eye[3] = {1, 2, 3}, at[3] = {0, 0, 0}, up[3] = {0, 1, 0};
    soc_mat4_look_at_rh(m, eye, at, up);
    soc_mat4_inverse(inv, m);
    soc_mat4_perspective_rh_no(m, 1.5707964f, 16.0f / 9.0f, 0.1f, 1000.0f);
    soc_mat4_ortho_rh_no(m, -16, 16, -16, 16, -100, 100);
    soc_mat4_mul(inv, m, inv);
}

void abi_introspection() {
    static const char* types[] = {"soc_globals", "soc_img", "soc_frame_images", "soc_auto_exposure", "soc_mesh",
                                  "soc_material", "soc_pass_desc", "soc_camera", "soc_entity", "no_such_type"};
    for (const char* t : types) (void)soc_abi_sizeof(t);
    expect(soc_abi_offsetof("soc_globals", "resolution") >= 0, "offsetof");
    expect(soc_abi_offsetof("soc_globals", "no_such_field") == -1, "offsetof unknown");
    expect(soc_abi_version() == 1, "abi version");
}

void render_graph(const soc_globals& g, int W, int H) {
    // fake (never dereferenced) device pointers: graph construction makes no GPU call
    char* fake = reinterpret_cast<char*>(0x100000);
    auto im = [&](int w, int h, int fmt, int bpp) { return soc_img{fake, w, h, w * bpp, fmt}; };
    soc_frame_images fi;
    std::memset(&fi, 0, sizeof fi);
    fi.albedo = fi.emissive = fi.normal = fi.velocity = fi.color = im(W, H, SOC_FMT_RGBA16F, 8);
    fi.depth = im(W, H, SOC_FMT_D32F, 4);
    fi.shadow = im(4096, 4096, SOC_FMT_D32F, 4);
    fi.noise = im(64, 64, SOC_FMT_RGBA8_UNORM, 4);
    for (int i = 0; i < 4; ++i) fi.bloom_mips[i] = im(W >> i, H >> i, SOC_FMT_RGBA16F, 8);
    fi.ssao = fi.ssao_blur = im(W / 2, H / 2, SOC_FMT_R8_UNORM, 1);
    fi.clouds = im(W, H, SOC_FMT_RGBA8_UNORM, 4);
    for (int i = 0; i < 2; ++i) fi.history_color[i] = fi.history_velocity[i] = im(W, H, SOC_FMT_RGBA16F, 8);
    fi.output = im(W, H, SOC_FMT_RGBA8_UNORM, 4);
    fi.auto_exposure = reinterpret_cast<soc_auto_exposure*>(fake);
    fi.d_globals = reinterpret_cast<soc_globals*>(fake);
    expect(soc_renderer_create(nullptr, 0) == nullptr, "create(null) rejected");
    for (uint32_t flags : {0u, (uint32_t)SOC_RENDERER_UNFUSED_BLOOM | SOC_RENDERER_UNFUSED_TONEMAP | SOC_RENDERER_UNFUSED_HISTOGRAM,
                           (uint32_t)SOC_RENDERER_NO_SKY_SPLIT, (uint32_t)SOC_RENDERER_EXACT_BLOOM}) {
        soc_renderer* r = soc_renderer_create(&fi, flags);
        expect(r != nullptr, "soc_renderer_create");
        if (!r) continue;
        int calls = 0;
        soc_pass_desc d;
        std::memset(&d, 0, sizeof d);
        d.name = "CallerPass";
        d.group = "Ambient Occlusion";
        d.phase = SOC_PHASE_PRE_EXPOSURE;
        d.read_count = 2;
        d.reads[0] = SOC_RES_SSAO;
        d.reads[1] = SOC_RES_COLOR;
        d.write_count = 1;
        d.writes[0] = SOC_RES_USER0 + 5;
        expect(soc_renderer_add_pass(r, &d, count_pass, &calls, "SSAOBlur") == SOC_OK, "add_pass");
        expect(soc_renderer_add_pass(r, &d, count_pass, &calls, nullptr) != SOC_OK, "duplicate name rejected");
        d.name = "Other";
        expect(soc_renderer_add_pass(r, &d, count_pass, &calls, "NoSuchPass") != SOC_OK, "unknown anchor rejected");
        d.reads[0] = 64;
        expect(soc_renderer_add_pass(r, &d, count_pass, &calls, nullptr) != SOC_OK, "bad resource rejected");
        d.reads[0] = SOC_RES_SSAO;
        d.phase = SOC_PHASE_POST_EXPOSURE;
        d.flags = SOC_PASS_ASYNC;
        expect(soc_renderer_add_pass(r, &d, count_pass, &calls, nullptr) == SOC_OK, "async post pass");
        // the library-owned ScreenSpaceReflection pass: argument errors, the default anchor, a duplicate, the rebuilds below
        const soc_img mr = im(W, H, SOC_FMT_RGBA16F, 8), ssr = im(W, H, SOC_FMT_RGBA16F, 8), none{};
        const int U = SOC_RES_USER0;
        expect(soc_renderer_add_screen_space_reflection(nullptr, mr, ssr, none, U, U + 1, 0, nullptr) != SOC_OK, "ssr: null renderer");
        expect(soc_renderer_add_screen_space_reflection(r, none, ssr, none, U, U + 1, 0, nullptr) != SOC_OK, "ssr: null image");
        expect(soc_renderer_add_screen_space_reflection(r, mr, ssr, none, SOC_RES_DEPTH, U + 1, 0, nullptr) != SOC_OK, "ssr: bad resource");
        expect(soc_renderer_add_screen_space_reflection(r, mr, ssr, none, U, U + 1, 0, "NoSuchPass") != SOC_OK, "ssr: unknown anchor");
        expect(soc_renderer_add_screen_space_reflection(r, mr, im(W / 2, H, SOC_FMT_RGBA16F, 8), none, U, U + 1, 0, nullptr) != SOC_OK,
               "ssr: extent mismatch");
        expect(soc_renderer_add_screen_space_reflection(r, mr, ssr, im(W, H, SOC_FMT_R8_UNORM, 1), U, U + 1, SOC_PASS_ASYNC, nullptr) == SOC_OK,
               "ssr: add");
        expect(soc_renderer_add_screen_space_reflection(r, mr, ssr, none, U, U + 1, 0, nullptr) != SOC_OK, "ssr: duplicate");
        expect(soc_screen_space_reflection(&g, none, none, none, none, none, none, nullptr) != SOC_OK, "ssr: null images");
        // the library-owned depth-of-field pair: the chain at a fake address of its own (the frame's colour may not alias
        // it); refused on a fused-histogram renderer, argument errors that leave the graph as it was, a duplicate
        const soc_img chain{fake + (1 << 28), W, H, W * 8, SOC_FMT_RGBA16F};
        const bool unfused = flags & SOC_RENDERER_UNFUSED_HISTOGRAM;
        expect(soc_depth_of_field_chain_bytes(W, H, W * 8) > (size_t)W * H * 8, "dof: chain bytes");
        expect(soc_depth_of_field_chain_bytes(W, H, W * 8 - 8) == 0 && soc_depth_of_field_chain_bytes(0, H, 8) == 0, "dof: bad chain");
        expect(soc_renderer_add_depth_of_field(nullptr, chain, U + 2, nullptr) != SOC_OK, "dof: null renderer");
        if (!unfused) {
            expect(soc_renderer_add_depth_of_field(r, chain, U + 2, nullptr) != SOC_OK, "dof: fused histogram refused");
        } else {
            expect(soc_renderer_add_depth_of_field(r, none, U + 2, nullptr) != SOC_OK, "dof: null chain");
            expect(soc_renderer_add_depth_of_field(r, mr, U + 2, nullptr) != SOC_OK, "dof: chain aliases the colour");
            expect(soc_renderer_add_depth_of_field(r, chain, SOC_RES_COLOR, nullptr) != SOC_OK, "dof: bad resource");
            expect(soc_renderer_add_depth_of_field(r, chain, U + 2, "NoSuchPass") != SOC_OK, "dof: unknown anchor");
            expect(soc_renderer_add_depth_of_field(r, chain, U + 2, "ToneMapping") != SOC_OK, "dof: anchor in the other phase");
            const int before_n = soc_renderer_pass_count(r);
            expect(soc_renderer_add_depth_of_field(r, soc_img{chain.data, W / 2, H, W * 4, SOC_FMT_RGBA16F}, U + 2, nullptr) != SOC_OK,
                   "dof: extent mismatch");
            expect(soc_renderer_pass_count(r) == before_n, "dof: refusals leave the graph");
            expect(soc_renderer_add_depth_of_field(r, chain, U + 2, nullptr) == SOC_OK, "dof: add");
            expect(soc_renderer_pass_count(r) == before_n + 2, "dof: two passes");
            expect(soc_renderer_add_depth_of_field(r, chain, U + 2, nullptr) != SOC_OK, "dof: duplicate");
        }
        expect(soc_depth_of_field_mips(none, none, nullptr) != SOC_OK, "dof mips: null images");
        expect(soc_depth_of_field_mips(mr, mr, nullptr) != SOC_OK, "dof mips: colour aliases the chain");
        expect(soc_depth_of_field(&g, none, none, none, nullptr) != SOC_OK, "dof: null images");
        expect(soc_depth_of_field(nullptr, fi.depth, chain, mr, nullptr) != SOC_OK, "dof: null globals");
        expect(soc_depth_of_field(&g, fi.depth, chain, chain, nullptr) != SOC_OK, "dof: target aliases the chain");
        soc_raster_scene sc;
        std::memset(&sc, 0, sizeof sc);
        sc.mesh.positions = sc.mesh.normals = sc.mesh.uvs = reinterpret_cast<const float*>(fake);
        sc.mesh.indices = reinterpret_cast<const uint32_t*>(fake);
        sc.mesh.vertex_count = 3;
        sc.mesh.triangle_count = 1;
        sc.materials = reinterpret_cast<const soc_material*>(fake);
        sc.material_count = 1;
        sc.visibility = reinterpret_cast<uint64_t*>(fake);
        sc.workspace = fake;
        sc.shadow = 1;
        expect(soc_renderer_set_raster_scene(r, &sc) == SOC_OK, "set_raster_scene");
        const int n = soc_renderer_pass_count(r);
        int32_t deps[64];
        for (int i = 0; i < n; ++i) {
            uint64_t rd = 0, wr = 0;
            expect(soc_renderer_pass_name(r, i) && soc_renderer_pass_group(r, i), "name / group");
            expect(soc_renderer_pass_uses(r, i, &rd, &wr) == SOC_OK, "uses");
            expect(soc_renderer_pass_dependencies(r, i, deps, 64) >= 0, "deps");
            expect(soc_renderer_pass_carry_dependencies(r, i, deps, 64) >= 0, "carry deps");
            expect(soc_renderer_pass_dependencies(r, i, nullptr, 0) >= 0, "deps count");
            (void)soc_renderer_pass_lane(r, i);
            expect(soc_renderer_pass_ms(r, i) < 0.0f, "no timing recorded");
        }
        expect(soc_renderer_pass_dependencies(r, n, deps, 64) < 0, "out-of-range index rejected");
        char buf[4096];
        expect(soc_renderer_metrics_json(r, 0, buf, sizeof buf) > 0, "metrics json");
        expect(soc_renderer_metrics_json(r, 0, buf, 8) > 8, "metrics json truncated");
        // the frame planner through its test hook (no GPU call): the first one-call frame over the raster head and the
        // caller passes and the frame after it, then a frame split into its two phases
        char plan[8192];
        for (int k = 0; k < 2; ++k)
            expect(soc_debug_plan_frame(r, &g, SOC_PHASE_ALL, k, 1, plan, sizeof plan) > 0, "plan: one-call frame");
        expect(std::strstr(plan, "run\tGBufferGeneration\t0\t") != nullptr, "plan: runs the raster head");
        expect(soc_debug_plan_frame(r, &g, SOC_PHASE_PRE_EXPOSURE, 0, 1, plan, 16) > 16, "plan: PRE phase, truncated");
        expect(soc_debug_plan_frame(r, &g, SOC_PHASE_POST_EXPOSURE, 0, 0, nullptr, 0) > 0, "plan: POST phase, length only");
        expect(soc_debug_plan_frame(r, nullptr, SOC_PHASE_ALL, 0, 0, plan, sizeof plan) < 0, "plan: null globals rejected");
        expect(soc_renderer_set_raster_scene(r, nullptr) == SOC_OK, "clear raster scene");
        expect(soc_renderer_set_exposure_pixels(r, (uint64_t)W * H * 8, 1) == SOC_OK, "exposure pixels");
        soc_renderer_destroy(r);
    }
}

// The clouds planner through its test hook (no GPU call; fake, never dereferenced addresses): the single-kernel form, a
// renderer's frames on one state (primed and built, then cached, then another sun), the per-call form above 1440p, a
// frame without a sky table, the refusals, a truncated buffer and the length-only call.
void clouds_plan(const soc_globals& g0, int W, int H) {
    char* fake = reinterpret_cast<char*>(0x10000000);
    soc_globals g = g0;
    const soc_img depth{fake, W, H, W * 4, SOC_FMT_D32F}, target{fake + (1 << 28), W, H, W * 4, SOC_FMT_RGBA8_UNORM};
    const soc_img noise{fake + (2 << 28), 64, 64, 256, SOC_FMT_RGBA8_UNORM}, r8{fake + (2 << 28), 64, 64, 64, SOC_FMT_R8_UNORM};
    void* ws = fake + (3 << 28);
    const int32_t res[6] = {1531, 1543, 769, 773, 787, 1277};
    std::vector<uint8_t> state(soc_debug_cloud_state_bytes(), 0);
    char buf[2048];
    expect(soc_debug_plan_clouds(&g, depth, r8, target, nullptr, 0, res, nullptr, buf, sizeof buf) > 0 &&
               std::strstr(buf, "kernel\tclouds_kernel\tr8\t") != nullptr, "clouds plan: single kernel");
    expect(soc_debug_plan_clouds(&g, depth, noise, target, ws, 0, res, state.data(), buf, sizeof buf) > 0 &&
               std::strstr(buf, "memset\tcounter1\t256\n") != nullptr, "clouds plan: first frame primes the blocks");
    expect(soc_debug_plan_clouds(&g, depth, noise, target, ws, 1, res, state.data(), buf, sizeof buf) > 0 &&
               std::strstr(buf, "clouds_od_lut") == nullptr && std::strstr(buf, "\tcounter=1\tzero=0\t") != nullptr,
           "clouds plan: second frame is cached");
    g.sun_info.direction[1] *= 0.5f;
    expect(soc_debug_plan_clouds(&g, depth, noise, target, ws, 0, res, state.data(), buf, sizeof buf) > 0 &&
               std::strstr(buf, " od=1 noise=0 ") != nullptr, "clouds plan: another sun rebuilds the od table");
    const soc_img big{fake + (1 << 28), 2562, 1440, 2562 * 4, SOC_FMT_RGBA8_UNORM}, bigd{fake, 2562, 1440, 2562 * 4, SOC_FMT_D32F};
    g.resolution[0] = 2562;
    g.resolution[1] = 1440;
    expect(soc_debug_plan_clouds(&g, bigd, noise, big, ws, 1, res, state.data(), buf, sizeof buf) > 0 &&
               std::strstr(buf, "\tzero=-1\t") != nullptr, "clouds plan: sky-bound above 1440p builds per call");
    g.camera_position[1] = -1500.0f;
    expect(soc_debug_plan_clouds(&g, bigd, noise, big, ws, 0, res, nullptr, buf, sizeof buf) > 0 &&
               std::strstr(buf, "clouds_sky_table") == nullptr, "clouds plan: no sky table below the surface");
    expect(soc_debug_plan_clouds(&g, bigd, noise, big, ws, 0, res, nullptr, buf, 16) > 16 && std::strlen(buf) == 15,
           "clouds plan: truncated");
    expect(soc_debug_plan_clouds(&g, bigd, noise, big, ws, 0, res, nullptr, nullptr, 0) > 0, "clouds plan: length only");
    expect(soc_debug_plan_clouds(nullptr, depth, noise, target, ws, 0, res, state.data(), buf, sizeof buf) == SOC_E_INVALID_ARG,
           "clouds plan: null globals");
    expect(soc_debug_plan_clouds(&g, target, noise, target, ws, 0, res, nullptr, buf, sizeof buf) == SOC_E_INVALID_ARG,
           "clouds plan: depth format");
    expect(soc_debug_plan_clouds(&g, depth, depth, target, ws, 0, res, nullptr, buf, sizeof buf) == SOC_E_UNSUPPORTED,
           "clouds plan: noise format");
    const soc_img small{fake + (2 << 28), 64, 32, 256, SOC_FMT_RGBA8_UNORM};
    expect(soc_debug_plan_clouds(&g, depth, small, target, ws, 0, res, state.data(), buf, sizeof buf) == SOC_E_SHAPE &&
               std::strstr(buf, "state\tod=0\tnoise=0\t") == buf, "clouds plan: noise extent, the state reset");
    expect(soc_debug_plan_clouds(&g, depth, noise, target, ws, 0, nullptr, nullptr, buf, sizeof buf) == SOC_E_INVALID_ARG,
           "clouds plan: null residency");
    g.resolution[0] = 0;
    expect(soc_debug_plan_clouds(&g, depth, noise, target, ws, 0, res, nullptr, buf, sizeof buf) == 0, "clouds plan: empty extent");
}

// The Composition planner through its test hook (no GPU call; fake, never dereferenced addresses): each entry point's
// call on the pair and the generic path, the render graph's forms, SkyCompose, each rejection, a truncated buffer and the
// length-only call.
void composition_plan(const soc_globals& g0) {
    enum { HIST = 1, FOLD = 2, SKY_EXTERNAL = 4, BOUNDED = 8, CASCADED = 16, SKY_COMPOSE = 32 };
    char* fake = reinterpret_cast<char*>(0x10000000);
    const int S = 256;
    soc_globals g = g0;
    soc_sun_cascades rec;
    expect(soc_sun_cascades_from_sun(&g, S, &rec) == SOC_OK, "composition plan: a one-cascade record");
    auto* dg = reinterpret_cast<const soc_globals*>(fake + 0xa0000000u);
    auto* ae = reinterpret_cast<soc_auto_exposure*>(fake + 0xb0000000u);
    auto* scratch = reinterpret_cast<uint32_t*>(fake + 0xb1000000u);
    auto* counter = reinterpret_cast<uint32_t*>(fake + 0xb2000000u);
    const void* bounds = fake + 0xb3000000u;
    char buf[2048];
    struct Frame {
        soc_img im[8], mip1, mip3;
    };
    auto frame = [&](int W, int H) {
        Frame f;
        const int fmt[8] = {SOC_FMT_RGBA16F, SOC_FMT_RGBA16F, SOC_FMT_RGBA16F, SOC_FMT_RGBA16F, SOC_FMT_D32F, SOC_FMT_R8_UNORM,
                            SOC_FMT_D32F, SOC_FMT_RGBA8_UNORM};
        const int bpp[8] = {8, 8, 8, 8, 4, 1, 4, 4};
        for (int i = 0; i < 8; ++i) {
            const int w = i == 5 ? (W + 1) / 2 : i == 6 ? S : W, h = i == 5 ? (H + 1) / 2 : i == 6 ? S : H;
            f.im[i] = soc_img{fake + ((size_t)i << 28), w, h, w * bpp[i], fmt[i]};
        }
        f.mip1 = soc_img{fake + (8u << 28), W / 2, H / 2, W / 2 * 8, SOC_FMT_RGBA16F};
        f.mip3 = soc_img{fake + 0x90000000u, W / 8, H / 8, W / 8 * 8, SOC_FMT_RGBA16F};
        return f;
    };
    auto plan = [&](const Frame& f, uint32_t what, uint32_t flags = 0, uint32_t* n = nullptr, const soc_img* m1 = nullptr,
                    const soc_img* m3 = nullptr, const soc_sun_cascades* cs = nullptr) {
        return soc_debug_plan_composition(&g, dg, f.im, what, ae, scratch, m1, m3, bounds, flags, n, cs, buf, sizeof buf);
    };
    auto has = [&](const char* text) { return std::strstr(buf, text) != nullptr; };
    g.point_light_count = 3;
    g.spot_light_count = 2;
    for (int pair = 1; pair >= 0; --pair) {
        const Frame f = pair ? frame(64, 48) : frame(97, 55);
        g.resolution[0] = f.im[0].width;
        g.resolution[1] = f.im[0].height;
        const char* path = pair ? "composition\tpair\t" : "composition\tgeneric\t";
        expect(plan(f, 0) > 0 && has(path), "composition plan: soc_composition");
        expect(plan(f, BOUNDED, SOC_LIGHTS_CULL, counter) > 0 && has(pair ? " lb=7 " : "composition_generic_bounded"),
               "composition plan: soc_composition_bounded");
        expect(plan(f, CASCADED, 0, nullptr, nullptr, nullptr, &rec) > 0 && has(pair ? " cs=1\t" : "composition_generic_cascaded"),
               "composition plan: soc_composition_cascaded");
        expect(plan(f, HIST | FOLD) > 0 && has(pair ? "histogram_fold" : "pass\tgenerate_luminance_histogram"),
               "composition plan: soc_composition_luminance_histogram");
        expect(plan(f, HIST | FOLD | BOUNDED) > 0 && has(pair ? " lb=1 " : "pass\t"),
               "composition plan: soc_composition_luminance_histogram_bounded");
        expect(plan(f, HIST | FOLD | CASCADED, 0, nullptr, nullptr, nullptr, &rec) > 0 && has("\tcascades=1,256:"),
               "composition plan: soc_composition_luminance_histogram_cascaded");
        // 97 clouds texels a row are no multiple of 8 bytes: the per-pixel form
        expect(plan(f, SKY_COMPOSE) > 0 && has(pair ? "sky_compose_pair\tcp=1" : "sky_compose_pair\tcp=0"), "composition plan: SkyCompose");
        if (pair) {   // the render graph's forms
            expect(plan(f, HIST | SKY_EXTERNAL | BOUNDED, SOC_LIGHTS_CULL, nullptr, &f.mip1, &f.mip3) > 0 &&
                       has(" bl=1 sp=1 lb=3 ") && !has("histogram_fold"), "composition plan: the render graph's call");
            expect(plan(f, HIST | BOUNDED, 0, counter, &f.mip1) == SOC_E_INVALID_ARG, "composition plan: the counter with the in-kernel bloom");
            expect(plan(f, HIST | CASCADED, 0, nullptr, &f.mip1, nullptr, &rec) == SOC_E_UNSUPPORTED, "composition plan: cascades with mip1");
            expect(plan(f, HIST | CASCADED, 0, nullptr, nullptr, &f.mip3, &rec) == SOC_E_UNSUPPORTED, "composition plan: cascades with mip3");
            expect(plan(f, HIST, 0, nullptr, &f.im[0]) == SOC_E_SHAPE, "composition plan: mip1 extent");
            expect(plan(f, HIST, 0, nullptr, nullptr, &f.im[0]) == SOC_E_SHAPE, "composition plan: mip3 extent");
            expect(plan(f, 0, 0, nullptr, &f.mip1) == SOC_E_SHAPE, "composition plan: mip1 without the histogram");
        } else {      // the three errors after a failed fusion
            expect(plan(f, HIST, 0, nullptr, nullptr, &f.mip3) == SOC_E_SHAPE, "composition plan: zero cells off the pair path");
            expect(plan(f, HIST, 0, nullptr, &f.mip1) == SOC_E_SHAPE, "composition plan: in-kernel bloom off the pair path");
            expect(plan(f, HIST | SKY_EXTERNAL) == SOC_E_INVALID_ARG, "composition plan: sky_external off the pair path");
        }
        expect(plan(f, SKY_EXTERNAL) == SOC_E_INVALID_ARG, "composition plan: sky_external without the histogram");
        expect(plan(f, BOUNDED, 2) == SOC_E_INVALID_ARG, "composition plan: unknown flags");
        expect(plan(f, CASCADED | BOUNDED, 0, nullptr, nullptr, nullptr, &rec) == SOC_E_UNSUPPORTED, "composition plan: cascades with bounds");
        expect(plan(f, CASCADED) == SOC_E_INVALID_ARG, "composition plan: null cascades");
        soc_sun_cascades bad = rec;
        bad.count = 5;
        expect(plan(f, CASCADED, 0, nullptr, nullptr, nullptr, &bad) == SOC_E_INVALID_ARG, "composition plan: cascades count");
        for (int i = 0; i < 8; ++i) {
            Frame b = f;
            b.im[i].format = i == 4 || i == 6 ? SOC_FMT_RGBA16F : SOC_FMT_D32F;
            expect(plan(b, HIST | FOLD) == SOC_E_INVALID_ARG, "composition plan: an image's format");
        }
        expect(soc_debug_plan_composition(&g, dg, f.im, 0, ae, scratch, nullptr, nullptr, bounds, 0, nullptr, nullptr, buf, 16) > 16 &&
                   std::strlen(buf) == 15, "composition plan: truncated");
        expect(soc_debug_plan_composition(&g, dg, f.im, HIST, ae, scratch, nullptr, nullptr, bounds, 0, nullptr, nullptr, nullptr, 0) > 0,
               "composition plan: length only");
        expect(soc_debug_plan_composition(&g, nullptr, f.im, 0, ae, scratch, nullptr, nullptr, bounds, 0, nullptr, nullptr, buf, sizeof buf) ==
                   SOC_E_INVALID_ARG, "composition plan: lights without device globals");
        expect(soc_debug_plan_composition(&g, dg, f.im, BOUNDED, ae, scratch, nullptr, nullptr, nullptr, 0, nullptr, nullptr, buf, sizeof buf) ==
                   SOC_E_INVALID_ARG, "composition plan: bounded without bounds");
        expect(soc_debug_plan_composition(nullptr, dg, f.im, 0, ae, scratch, nullptr, nullptr, bounds, 0, nullptr, nullptr, buf, sizeof buf) ==
                   SOC_E_INVALID_ARG, "composition plan: null globals");
        expect(soc_debug_plan_composition(&g, dg, f.im, HIST, nullptr, scratch, nullptr, nullptr, bounds, 0, nullptr, nullptr, buf, sizeof buf) ==
                   SOC_E_INVALID_ARG, "composition plan: null auto exposure");
        expect(soc_debug_plan_composition(&g, dg, f.im, SKY_COMPOSE, ae, nullptr, nullptr, nullptr, bounds, 0, nullptr, nullptr, buf, sizeof buf) ==
                   SOC_E_INVALID_ARG, "composition plan: SkyCompose without scratch");
        expect(soc_debug_plan_composition(&g, dg, nullptr, 0, ae, scratch, nullptr, nullptr, bounds, 0, nullptr, nullptr, buf, sizeof buf) ==
                   SOC_E_INVALID_ARG, "composition plan: null images");
    }
}

// The TAA, SSAO and bloom planners through their test hook (no GPU call; fake, never dereferenced addresses): the
// accepted cases of tests/test_post_plan.py (every kernel family, the extents, the views and the tone-map outputs), every
// rejection of the entry points, a truncated buffer and the length-only call.
void post_plans(const soc_globals& g0) {
    enum { TAA, TAA_TM, SSAO, SSAO_BLUR, SSAO_NOISE, BLOOM_W, BLOOM_DOWN, BLOOM_UP, SPARSE = 256 };
    char* fake = reinterpret_cast<char*>(0x10000000);
    const void* aux = fake + 0xc1000000u;
    const int32_t resident[6] = {24, 24, 24, 24, 24, 24};
    soc_globals g = g0;
    char buf[2048];
    auto image = [&](int i, int w, int h, int fmt) {
        const int bpp = fmt == SOC_FMT_RGBA16F ? 8 : fmt == SOC_FMT_R8_UNORM ? 1 : 4;
        return soc_img{fake + ((size_t)i << 28), w, h, w * bpp, fmt};
    };
    auto has = [&](const char* text) { return std::strstr(buf, text) != nullptr; };
    auto plan = [&](int pass, const soc_img* im, int n, int arg = 0, const void* a = nullptr, const soc_globals* gl = nullptr) {
        return soc_debug_plan_post(pass, gl ? gl : &g, im, n, a, arg, resident, buf, sizeof buf);
    };
    // TAA: target, colour, history, velocity, velocity history, depth, velocity_history_out, output
    struct Taa { soc_img im[8]; };
    auto taa = [&](int W, int H) {
        Taa t;
        for (int i = 0; i < 8; ++i) t.im[i] = image(i, W, H, i == 5 ? SOC_FMT_D32F : i == 7 ? SOC_FMT_RGBA8_UNORM : SOC_FMT_RGBA16F);
        g.resolution[0] = W;
        g.resolution[1] = H;
        return t;
    };
    for (int tm = 0; tm < 2; ++tm) {
        const void* ae = tm ? aux : nullptr;
        const int n = 7 + tm;
        const int sizes[6][2] = {{64, 36}, {130, 58}, {97, 55}, {8192, 16}, {8194, 16}, {64, 256}};
        // 130 depth texels a row are no multiple of 16 bytes: the halo-lane pair kernel
        const char* kernel[6] = {"taa_lds", "taa_pair2", "taa_fast", "taa_lds", "taa_generic", "taa_lds"};
        for (int k = 0; k < 6; ++k) {
            Taa t = taa(sizes[k][0], sizes[k][1]);
            expect(plan(tm, t.im, n, 0, ae) > 0 && has(kernel[k]) && has("pass\ttone_mapping") == (tm && (k == 2 || k == 4)),
                   "post plan: TAA extents");
        }
        Taa t = taa(64, 36);
        Taa v = t;
        v.im[5].data = fake + (5u << 28) + 8;   // a depth base 8 bytes off
        expect(plan(tm, v.im, n, 0, ae) > 0 && has("taa_pair2\t") && has("nbr=2"), "post plan: TAA depth offset");
        for (int i : {0, 1, 3, 6}) {   // each misaligned in turn
            v = t;
            v.im[i].data = fake + ((size_t)i << 28) + 8;
            expect(plan(tm, v.im, n, 0, ae) > 0 && has("taa_fast"), "post plan: TAA misaligned view");
        }
        v = t;
        v.im[1].width = v.im[1].height = 18;   // another colour extent
        v.im[1].pitch_bytes = 18 * 8;
        expect(plan(tm, v.im, n, 0, ae) > 0 && has("taa_generic"), "post plan: TAA generic");
        v = t;
        v.im[1].pitch_bytes = 1 << 23;   // past the pair kernels' 32-bit offsets
        expect(plan(tm, v.im, n, 0, ae) > 0 && has("taa_fast"), "post plan: TAA range");
        v = t;
        v.im[6] = soc_img{};
        expect(plan(tm, v.im, n, 0, ae) > 0 && has("vel_out=0"), "post plan: TAA without velocity_history_out");
        for (uint32_t fc : {0u, 5u}) {
            g.frame_counter = fc;
            expect(plan(tm, t.im, n, 0, ae) > 0, "post plan: TAA frame counter");
        }
        // rejections
        expect(soc_debug_plan_post(tm, nullptr, t.im, n, ae, 0, resident, buf, sizeof buf) == SOC_E_INVALID_ARG, "post plan: TAA null globals");
        for (int i = 0; i < 7; ++i) {
            v = t;
            v.im[i].format = SOC_FMT_R8_UNORM;
            expect(plan(tm, v.im, n, 0, ae) == SOC_E_INVALID_ARG, "post plan: TAA image format");
        }
        for (int i : {1, 2}) {
            v = t;
            v.im[i].data = t.im[0].data;
            expect(plan(tm, v.im, n, 0, ae) == SOC_E_INVALID_ARG, "post plan: TAA target aliases an input");
        }
        for (int i : {3, 4}) {
            v = t;
            v.im[6].data = t.im[i].data;
            expect(plan(tm, v.im, n, 0, ae) == SOC_E_INVALID_ARG, "post plan: TAA velocity_history_out aliases");
        }
        v = t;
        v.im[6].width = 32;
        expect(plan(tm, v.im, n, 0, ae) == SOC_E_SHAPE, "post plan: TAA velocity_history_out extent");
        if (tm) {
            expect(plan(TAA_TM, t.im, 8, 0, nullptr) == SOC_E_INVALID_ARG, "post plan: TAA null auto exposure");
            const int fmts[3] = {SOC_FMT_RGBA8_SRGB, SOC_FMT_RGBA16F, SOC_FMT_RGBA8_UNORM};
            for (int k = 0; k < 3; ++k) {
                v = t;
                v.im[7] = image(7, 64, 36, fmts[k]);
                expect(plan(TAA_TM, v.im, 8, 0, ae) > 0 && has("tm=1 sf=1") == (k != 1) && has("pass\t") == (k == 1), "post plan: TAA output format");
            }
            v = t;
            v.im[7].data = fake + (7u << 28) + 4;
            expect(plan(TAA_TM, v.im, 8, 0, ae) > 0 && has("pass\ttone_mapping"), "post plan: TAA misaligned output");
            v.im[7] = t.im[0];   // aliases the target: two passes
            expect(plan(TAA_TM, v.im, 8, 0, ae) > 0 && has("pass\ttone_mapping"), "post plan: TAA output aliases the target");
            v.im[7].width = 0;
            expect(plan(TAA_TM, v.im, 8, 0, ae) == SOC_E_INVALID_ARG, "post plan: TAA bad output");
        }
        expect(soc_debug_plan_post(tm, &g, t.im, n, ae, 0, resident, buf, 16) > 16 && std::strlen(buf) == 15, "post plan: truncated");
        expect(soc_debug_plan_post(tm, &g, t.im, n, ae, 0, resident, nullptr, 0) > 0, "post plan: length only");
        expect(soc_debug_plan_post(tm, &g, t.im, n - 1, ae, 0, resident, buf, sizeof buf) == SOC_E_INVALID_ARG, "post plan: too few images");
    }
    expect(soc_debug_plan_post(8, &g, nullptr, 0, nullptr, 0, resident, buf, sizeof buf) == SOC_E_INVALID_ARG, "post plan: unknown pass");
    // SSAO: depth, normal, target
    const int frames[3][2] = {{128, 72}, {260, 130}, {97, 55}};
    for (int k = 0; k < 3; ++k)
        for (int table = 0; table < 2; ++table) {
            const int W = frames[k][0], H = frames[k][1];
            soc_img im[3] = {image(0, W, H, SOC_FMT_D32F), image(1, W, H, SOC_FMT_RGBA16F), image(2, W / 2, H / 2, SOC_FMT_R8_UNORM)};
            g = g0;
            expect(plan(SSAO, im, 3, 0, table ? aux : nullptr) > 0 && has(table ? "ssao_pipe_kernel" : "ssao_kernel\ttable=0 sip=1 full=1"),
                   "post plan: SSAO generation");
            for (int ks : {8, 40}) {
                g.ssao_kernel_size = ks;
                expect(plan(SSAO, im, 3, 0, table ? aux : nullptr) > 0 && has(ks == 40 ? (table ? "ssao_pipe_kernel" : "full=1") : "full=0"),
                       "post plan: SSAO kernel size");
            }
            g = g0;
            g.camera_projection_matrix[11] = -0.5f;
            expect(plan(SSAO, im, 3, 0, table ? aux : nullptr) > 0 && has("persp=1") == false, "post plan: SSAO projection w row");
            g = g0;
            g.camera_inverse_projection_matrix[2] = 0.125f;
            expect(plan(SSAO, im, 3, 0, table ? aux : nullptr) > 0 && has("sip=0"), "post plan: SSAO dense inverse projection");
            g = g0;
            g.ssao_radius = 0.0f;
            expect(plan(SSAO, im, 3, 0, table ? aux : nullptr) > 0 && has("sip=0"), "post plan: SSAO radius 0");
            g = g0;
            soc_img bad[3] = {im[0], im[1], im[2]};
            bad[0].width = bad[0].height = 1;
            bad[0].pitch_bytes = 4;
            expect(plan(SSAO, bad, 3, 0, aux) == SOC_E_SHAPE, "post plan: SSAO depth 1x1");
            bad[0] = im[0];
            bad[0].pitch_bytes = 1 << 23;
            expect(plan(SSAO, bad, 3, 0, aux) == SOC_E_SHAPE, "post plan: SSAO range");
            for (int i = 0; i < 3; ++i) {
                soc_img b2[3] = {im[0], im[1], im[2]};
                b2[i].format = SOC_FMT_RGBA8_UNORM;
                expect(plan(SSAO, b2, 3, 0, aux) == SOC_E_INVALID_ARG, "post plan: SSAO image format");
            }
            expect(soc_debug_plan_post(SSAO, nullptr, im, 3, aux, 0, resident, buf, sizeof buf) == SOC_E_INVALID_ARG, "post plan: SSAO null globals");
            soc_img blur[2] = {im[2], image(3, W / 2, H / 2, SOC_FMT_R8_UNORM)};
            expect(plan(SSAO_BLUR, blur, 2) > 0 && has("ssao_blur_kernel"), "post plan: SSAO blur");
            blur[1] = image(3, W, H, SOC_FMT_R8_UNORM);
            expect(plan(SSAO_BLUR, blur, 2) > 0 && has("ssao_blur_generic"), "post plan: SSAO blur, unequal extents");
            blur[1] = blur[0];
            expect(plan(SSAO_BLUR, blur, 2) == SOC_E_INVALID_ARG, "post plan: SSAO blur aliased");
            blur[1].format = SOC_FMT_D32F;
            expect(plan(SSAO_BLUR, blur, 2) == SOC_E_INVALID_ARG, "post plan: SSAO blur format");
            soc_img noise[2] = {im[1], im[2]};
            expect(plan(SSAO_NOISE, noise, 2, 0, aux) > 0 && has("ssao_noise_kernel"), "post plan: SSAO noise");
            expect(plan(SSAO_NOISE, noise, 2, 0, nullptr) == SOC_E_INVALID_ARG, "post plan: SSAO noise null table");
            noise[1].height = 0;
            expect(plan(SSAO_NOISE, noise, 2, 0, aux) == SOC_E_INVALID_ARG, "post plan: SSAO noise extents");
        }
    // weighted bloom: emissive, output, four mips
    const int extents[2][2] = {{64, 48}, {200, 104}};
    for (int k = 0; k < 2; ++k) {
        const int W = extents[k][0], H = extents[k][1];
        soc_img im[6] = {image(0, W, H, SOC_FMT_RGBA16F), image(1, W, H, SOC_FMT_RGBA16F)};
        for (int i = 0; i < 4; ++i) im[2 + i] = image(2 + i, W >> i, H >> i, SOC_FMT_RGBA16F);
        for (int stage = 0; stage <= 4; ++stage)
            for (int r : {8, 24, 4096}) {
                const int32_t res[6] = {r, r, r, r, r, r};
                expect(soc_debug_plan_post(BLOOM_W, &g, im, 6, nullptr, stage, res, buf, sizeof buf) > 0 &&
                           has("bloomw_down01p") == (stage <= 1) && has("bloomw_up10r") == (stage == 0 || stage == 4), "post plan: bloom stages");
            }
        expect(plan(BLOOM_W, im, 6, 4 | SPARSE) > 0 && has("zs=1 sparse=1"), "post plan: sparse bloom output");
        expect(soc_debug_plan_post(BLOOM_W, &g, im, 6, nullptr, 1, nullptr, buf, sizeof buf) == SOC_E_INVALID_ARG, "post plan: bloom null resident sets");
        expect(plan(BLOOM_W, im, 6, 5) == SOC_E_INVALID_ARG, "post plan: bloom stage");
        expect(plan(BLOOM_W, im, 2, 0) == SOC_E_INVALID_ARG, "post plan: bloom null mips");
        expect(plan(BLOOM_W, im, 5, 0) == SOC_E_UNSUPPORTED, "post plan: bloom three mips");
        soc_img bad[6];
        for (int i = 0; i < 6; ++i) {
            std::memcpy(bad, im, sizeof bad);
            bad[i].format = SOC_FMT_RGBA8_UNORM;
            expect(plan(BLOOM_W, bad, 6, 0) == SOC_E_INVALID_ARG, "post plan: bloom image format");
        }
        std::memcpy(bad, im, sizeof bad);
        bad[1].data = im[3].data;
        expect(plan(BLOOM_W, bad, 6, 0) == SOC_E_INVALID_ARG && plan(BLOOM_W, bad, 6, 2) > 0, "post plan: bloom output aliases mip 1");
        std::memcpy(bad, im, sizeof bad);
        bad[5].height += 1;
        expect(plan(BLOOM_W, bad, 6, 0) == SOC_E_UNSUPPORTED, "post plan: bloom chain that does not halve");
        // per-pass: same extent, exact half, other, forced generic; both sides of the quad bound
        for (int up = 0; up < 2; ++up) {
            const int pass = up ? BLOOM_UP : BLOOM_DOWN;
            const soc_img hi = im[2], same = image(6, W, H, SOC_FMT_RGBA16F), half = im[3], other = image(6, W / 2 + 1, H / 2, SOC_FMT_RGBA16F);
            soc_img p[2] = {hi, same};
            expect(plan(pass, p, 2) > 0 && has(up ? "bloom_up_same_q" : "bloom_down_same_q"), "post plan: bloom pass, same extent");
            expect(plan(pass, p, 2, 1) > 0 && has("_generic"), "post plan: bloom pass, forced generic");
            p[up ? 1 : 0] = hi;
            p[up ? 0 : 1] = half;
            expect(plan(pass, p, 2) > 0 && has(up ? "bloom_up_double\t" : "bloom_down_half_w"), "post plan: bloom pass, exact half");
            p[up ? 0 : 1] = other;
            expect(plan(pass, p, 2) > 0 && has("_generic"), "post plan: bloom pass, other ratio");
            p[1] = p[0];
            expect(plan(pass, p, 2) == SOC_E_INVALID_ARG, "post plan: bloom pass aliased");
            p[1] = same;
            p[1].format = SOC_FMT_D32F;
            expect(plan(pass, p, 2) == SOC_E_INVALID_ARG, "post plan: bloom pass format");
        }
    }
    soc_img q[2] = {image(0, 512, 512, SOC_FMT_RGBA16F), image(1, 1024, 1024, SOC_FMT_RGBA16F)};
    expect(plan(BLOOM_UP, q, 2) > 0 && has("bloom_up_double_q"), "post plan: the quad upsample at 2^20 pixels");
    q[0].height = 511;
    q[1].height = 1022;
    expect(plan(BLOOM_UP, q, 2) > 0 && has("bloom_up_double\t"), "post plan: one pixel per lane below it");
}

void writers(int W, int H) {
    HostImg rgba(W, H, SOC_FMT_RGBA8_UNORM, 4, 200);
    HostImg half(W, H, SOC_FMT_RGBA16F, 8);
    fill_rgba16f(half, 7, -4.0f, 70000.0f);   // includes overflow to inf
    const char* dir = std::getenv("SAN_TMP") ? std::getenv("SAN_TMP") : "/tmp";
    char path[512];
    std::snprintf(path, sizeof path, "%s/san_host.png", dir);
    expect(soc_write_png(path, rgba.data.data(), W, H, W * 4) == SOC_OK, "png");
    std::snprintf(path, sizeof path, "%s/san_host.exr", dir);
    expect(soc_write_exr(path, half.data.data(), W, H, W * 8) == SOC_OK, "exr");
    expect(soc_write_png("/nonexistent-dir/x.png", rgba.data.data(), W, H, W * 4) != SOC_OK, "png bad path");
}

void oracle_frame(const soc_globals& g0, int W, int H) {
    soc_globals g = g0;
    g.resolution[0] = W;
    g.resolution[1] = H;
    HostImg albedo(W, H, SOC_FMT_RGBA16F, 8), emissive(W, H, SOC_FMT_RGBA16F, 8), normal(W, H, SOC_FMT_RGBA16F, 8),
        velocity(W, H, SOC_FMT_RGBA16F, 8), depth(W, H, SOC_FMT_D32F, 4);
    expect(soc_scene_gbuffer(0, &g, W, H, (uint16_t*)albedo.data.data(), (uint16_t*)emissive.data.data(),
                             (uint16_t*)normal.data.data(), (float*)depth.data.data(), (uint16_t*)velocity.data.data()) == 0,
           "scene gbuffer");
    const int S = 128;
    HostImg shadow(S, S, SOC_FMT_D32F, 4);
    for (size_t i = 0; i < shadow.data.size() / 4; ++i) reinterpret_cast<float*>(shadow.data.data())[i] = 1.0f;
    expect(soc_scene_shadow(0, &g, S, (float*)shadow.data.data()) == 0, "scene shadow");
    HostImg noise(64, 64, SOC_FMT_RGBA8_UNORM, 4);
    uint32_t seed = 11;
    for (auto& b : noise.data) b = (uint8_t)(lcg(seed) >> 24);
    std::vector<HostImg> mips;
    for (int i = 0; i < 4; ++i) mips.emplace_back(std::max(W >> i, 1), std::max(H >> i, 1), SOC_FMT_RGBA16F, 8);
    // bloom chain (renderer.cpp:1024-1062)
    expect(soc_oracle_bloom_downsample(&g, emissive.img, mips[0].img) == SOC_OK, "bloom down 0");
    for (int i = 0; i < 3; ++i) expect(soc_oracle_bloom_downsample(&g, mips[i].img, mips[i + 1].img) == SOC_OK, "bloom down");
    for (int i = 3; i > 0; --i) expect(soc_oracle_bloom_upsample(&g, mips[i].img, mips[i - 1].img) == SOC_OK, "bloom up");
    expect(soc_oracle_bloom_upsample(&g, mips[0].img, emissive.img) == SOC_OK, "bloom up 0");
    HostImg ssao(W / 2, H / 2, SOC_FMT_R8_UNORM, 1), blur(W / 2, H / 2, SOC_FMT_R8_UNORM, 1);
    expect(soc_oracle_ssao_generation(&g, depth.img, normal.img, ssao.img) == SOC_OK, "ssao");
    expect(soc_oracle_ssao_blur(&g, ssao.img, blur.img) == SOC_OK, "ssao blur");
    HostImg clouds(W, H, SOC_FMT_RGBA8_UNORM, 4), color(W, H, SOC_FMT_RGBA16F, 8);
    expect(soc_oracle_cloud_rendering(&g, depth.img, noise.img, clouds.img) == SOC_OK, "clouds");
    soc_globals gl = g;
    gl.point_light_count = 2;
    gl.spot_light_count = 2;
    expect(soc_oracle_composition(&gl, color.img, albedo.img, emissive.img, normal.img, depth.img, blur.img, shadow.img,
                                  clouds.img) == SOC_OK, "composition (lights)");
    expect(soc_oracle_composition(&g, color.img, albedo.img, emissive.img, normal.img, depth.img, blur.img, shadow.img,
                                  clouds.img) == SOC_OK, "composition");
    soc_auto_exposure ae;
    std::memset(&ae, 0, sizeof ae);
    expect(soc_oracle_generate_luminance_histogram(&g, color.img, &ae) == SOC_OK, "histogram");
    expect(soc_oracle_resolve_luminance_histogram(&g, &ae, 0, 0) == SOC_OK, "resolve");
    expect(soc_oracle_generate_luminance_histogram(&g, color.img, &ae) == SOC_OK, "histogram 2");
    expect(soc_oracle_resolve_luminance_histogram(&g, &ae, (uint64_t)W * H * 8, 1) == SOC_OK, "resolve wide");
    HostImg prev(W, H, SOC_FMT_RGBA16F, 8), pvel(W, H, SOC_FMT_RGBA16F, 8), resolved(W, H, SOC_FMT_RGBA16F, 8);
    fill_rgba16f(prev, 3, 0.0f, 2.0f);
    expect(soc_oracle_temporal_antialiasing(&g, resolved.img, color.img, prev.img, velocity.img, pvel.img, depth.img) == SOC_OK,
           "taa");
    for (int fmt : {SOC_FMT_RGBA8_UNORM, SOC_FMT_RGBA8_SRGB}) {
        HostImg out(W, H, fmt, 4);
        expect(soc_oracle_tone_mapping(&g, resolved.img, &ae, out.img) == SOC_OK, "tone map 8");
    }
    HostImg out16(W, H, SOC_FMT_RGBA16F, 8), out32(W, H, SOC_FMT_RGBA32F, 16);
    expect(soc_oracle_tone_mapping(&g, resolved.img, &ae, out16.img) == SOC_OK, "tone map 16f");
    expect(soc_oracle_tone_mapping(&g, resolved.img, &ae, out32.img) == SOC_OK, "tone map 32f");
    // Hi-Z (min and max pyramids) of the depth
    std::vector<HostImg> hiz;
    int hw = std::max(W / 2, 1), hh = std::max(H / 2, 1), levels = 0;
    while (levels < 6) { hiz.emplace_back(hw, hh, SOC_FMT_D32F, 4); ++levels; if (hw == 1 && hh == 1) break; hw = std::max(hw / 2, 1); hh = std::max(hh / 2, 1); }
    std::vector<soc_img> hz;
    for (auto& h : hiz) hz.push_back(h.img);
    expect(soc_oracle_generate_hiz(&g, depth.img, hz.data(), (int)hz.size(), 0) == SOC_OK, "hiz min");
    expect(soc_oracle_generate_hiz(&g, depth.img, hz.data(), (int)hz.size(), 1) == SOC_OK, "hiz max");
}

void oracle_raster(const soc_globals& g0, int W, int H) {
    soc_globals g = g0;
    int nv = 0, nt = 0;
    expect(soc_scene_mesh_counts(0, &nv, &nt) == 0, "mesh counts");
    std::vector<float> pos(3 * nv), nrm(3 * nv), uv(2 * nv);
    std::vector<uint32_t> idx(3 * nt), mat(nt);
    expect(soc_scene_mesh(0, &g, pos.data(), nrm.data(), uv.data(), idx.data(), mat.data()) == 0, "mesh");
    const int nm = soc_scene_material_count(0), T = 32;
    std::vector<uint8_t> tex((size_t)nm * T * T * 4);
    std::vector<float> em(3 * nm);
    expect(soc_scene_material_textures(0, &g, T, tex.data(), em.data()) == 0, "material textures");
    soc_mesh m;
    std::memset(&m, 0, sizeof m);
    m.positions = pos.data();
    m.normals = nrm.data();
    m.uvs = uv.data();
    m.indices = idx.data();
    m.materials = mat.data();
    m.vertex_count = nv;
    m.triangle_count = nt;
    for (int i = 0; i < 4; ++i) m.model_matrix[i * 5] = m.normal_matrix[i * 5] = 1.0f;
    std::vector<soc_material> mats(nm);
    for (int i = 0; i < nm; ++i) {
        std::memset(&mats[i], 0, sizeof mats[i]);
        mats[i].albedo = soc_img{tex.data() + (size_t)i * T * T * 4, T, T, T * 4, SOC_FMT_RGBA8_SRGB};
        for (int k = 0; k < 4; ++k) mats[i].albedo_factor[k] = 1.0f;
        for (int k = 0; k < 3; ++k) mats[i].emissive_factor[k] = em[3 * i + k];
    }
    std::vector<uint64_t> vis((size_t)W * H, ~0ull);
    expect(soc_oracle_raster_visibility(&m, g.camera_projection_view_matrix, SOC_CULL_FRONT, vis.data(), W, H) == SOC_OK,
           "raster visibility");
    HostImg sh(64, 64, SOC_FMT_D32F, 4);
    for (size_t i = 0; i < sh.data.size() / 4; ++i) reinterpret_cast<float*>(sh.data.data())[i] = 1.0f;
    expect(soc_oracle_raster_depth(&m, g.sun_info.projection_view_matrix, SOC_CULL_BACK, 1.25f, 1.75f, sh.img) == SOC_OK,
           "raster depth");
    HostImg albedo(W, H, SOC_FMT_RGBA16F, 8), emissive(W, H, SOC_FMT_RGBA16F, 8), normal(W, H, SOC_FMT_RGBA16F, 8),
        velocity(W, H, SOC_FMT_RGBA16F, 8), depth(W, H, SOC_FMT_D32F, 4);
    expect(soc_oracle_gbuffer_resolve(&g, &m, mats.data(), nm, vis.data(), depth.img, albedo.img, emissive.img, normal.img,
                                      velocity.img) == SOC_OK, "gbuffer resolve");
    // mip chain of an odd-sized sRGB texture, packed after level 0
    const int TW = 37, TH = 5;
    const size_t bytes = soc_mip_chain_bytes(TW, TH, TW * 4);
    std::vector<uint8_t> chain(bytes, 128);
    expect(soc_oracle_generate_mips(soc_img{chain.data(), TW, TH, TW * 4, SOC_FMT_RGBA8_SRGB}) == SOC_OK, "mips");
    // terrain: heightmap -> normal map, tessellation
    const int HM = 64;
    std::vector<uint8_t> hm((size_t)HM * HM * 4);
    expect(soc_scene_terrain_heightmap(HM, hm.data()) == 0, "heightmap");
    HostImg hn(HM, HM, SOC_FMT_RGBA16F, 8);
    const soc_img hmi{hm.data(), HM, HM, HM * 4, SOC_FMT_RGBA8_UNORM};
    expect(soc_oracle_height_to_normal(hmi, hn.img) == SOC_OK, "height to normal");
    const int grid = 8, level = 3, nvert = ((grid - 1) * level + 1) * ((grid - 1) * level + 1), ntri = 2 * (grid - 1) * level * (grid - 1) * level;
    std::vector<float> tp(3 * nvert), tn(3 * nvert), tu(2 * nvert);
    std::vector<uint32_t> ti(3 * ntri);
    expect(soc_oracle_terrain_tessellate(&g, hmi, grid, level, tp.data(), tn.data(), tu.data(), ti.data()) == SOC_OK,
           "terrain tessellate");
    std::vector<uint16_t> tal((size_t)W * H * 4), tem((size_t)W * H * 4), tno((size_t)W * H * 4), tve((size_t)W * H * 4);
    std::vector<float> tde((size_t)W * H);
    expect(soc_scene_gbuffer(1, &g, W, H, tal.data(), tem.data(), tno.data(), tde.data(), tve.data()) == 0, "terrain gbuffer");
}

// Draw scenes and the raster workspaces (csrc/raster_host.cpp) over the paths that return before any HIP call: the two
// size functions against hand-computed layouts, every rejection of tests/test_draws_abi.py's
// test_host_validation_without_gpu with its code, and the release of scenes that were never built. The device pointers
// are fake and never dereferenced; the draw lists are real host arrays, which the checks do read.
soc_draw make_draw(int first_index, int triangles, int first_vertex, int vertices, int transform = 0, int material = 0) {
    return soc_draw{first_index, triangles, 0, first_vertex, vertices, transform, material};
}
soc_draw_scene make_scene(const std::vector<soc_draw>& draws) {
    const float* fake = reinterpret_cast<const float*>(256);
    soc_draw_scene sc;
    std::memset(&sc, 0, sizeof sc);
    sc.positions = sc.normals = sc.uvs = fake;
    sc.indices = reinterpret_cast<const uint32_t*>(256);
    sc.transforms = reinterpret_cast<const soc_transform*>(256);
    sc.workspace = reinterpret_cast<void*>(4096);
    sc.draws = draws.data();
    sc.draw_count = (int32_t)draws.size();
    sc.vertex_count = sc.index_count = 30;
    sc.transform_count = sc.material_count = 2;
    return sc;
}
bool mentions(const char* word) { return std::strstr(soc_last_error_string(), word) != nullptr; }

void draw_scenes(const soc_globals& g) {
    // [3 float4 -> 256] [counter 256] [1 entry -> 256] [3 x 64 B of vertex data]
    expect(soc_raster_workspace_size(3, 1) == 256 + 256 + 256 + 192, "raster workspace: 3 vertices, 1 triangle");
    expect(soc_raster_workspace_size(30, 10) == 512 + 256 + 256 + 1920, "raster workspace: 30 vertices, 10 triangles");
    expect(soc_raster_workspace_size(-1, 1) == 0 && soc_raster_workspace_size(1, -1) == 0, "raster workspace: negative counts");
    const soc_draw ok = make_draw(0, 10, 0, 30, 1, 1);
    // the flag's 256 B, five tables of no bytes, then two views of an empty raster workspace (its counter's 256 B)
    expect(soc_draw_workspace_size(nullptr, 0) == 256 + 2 * 256, "draw workspace: empty list");
    // flag 256, slots 240 -> 256, uvs 256, indices 120 -> 256, materials 40 -> 256, one DrawRec 36 -> 256, then two views
    // of soc_raster_workspace_size(30, 10) = 2944 -> 3072
    expect(soc_draw_workspace_size(&ok, 1) == 6 * 256 + 2 * 3072, "draw workspace: one draw");
    expect(soc_draw_workspace_size(nullptr, 1) == 0 && soc_draw_workspace_size(&ok, -1) == 0, "draw workspace: null list, negative count");
    for (const soc_draw& bad : {make_draw(0, -1, 0, 30), make_draw(0, 10, 0, -30), make_draw(0, 10, -1, 30), make_draw(-3, 10, 0, 30)})
        expect(soc_draw_workspace_size(&bad, 1) == 0, "draw workspace: negative field");
    const soc_draw big[2] = {make_draw(0, 0x7FFFFFFF, 0, 3), make_draw(0, 0x7FFFFFFF, 0, 3)};
    expect(soc_draw_workspace_size(big, 2) == 0, "draw workspace: totals beyond int32");

    const std::vector<soc_draw> one{ok};
    expect(soc_draw_scene_build(nullptr, nullptr) == SOC_E_INVALID_ARG && mentions("soc_draw_scene_build"), "build: null scene");
    for (int field = 0; field < 4; ++field) {
        soc_draw_scene sc = make_scene(one);
        if (field == 0) sc.positions = nullptr;
        if (field == 1) sc.indices = nullptr;
        if (field == 2) sc.transforms = nullptr;
        if (field == 3) sc.workspace = nullptr;
        expect(soc_draw_scene_build(&sc, nullptr) == SOC_E_INVALID_ARG && mentions("soc_draw_scene_build"), "build: null field");
    }
    for (int k = 0; k < 7; ++k) {
        soc_draw_scene sc = make_scene(one);
        if (k == 0) sc.vertex_count = -1;
        if (k == 1) sc.index_count = -1;
        if (k == 2) sc.draw_count = -1;
        if (k == 3) sc.transform_count = 0;
        if (k == 4) sc.material_count = 0;
        if (k == 5) sc.workspace = reinterpret_cast<void*>(4096 + 64);
        if (k == 6) sc.draws = nullptr;
        expect(soc_draw_scene_build(&sc, nullptr) == SOC_E_INVALID_ARG, "build: bad count, misaligned workspace or null draws");
    }
    for (const soc_draw& bad : {make_draw(0, -1, 0, 30), make_draw(-1, 10, 0, 30), make_draw(0, 10, -1, 30), make_draw(0, 10, 0, -1)}) {
        const std::vector<soc_draw> ds{ok, bad};
        const soc_draw_scene sc = make_scene(ds);
        expect(soc_draw_scene_build(&sc, nullptr) == SOC_E_INVALID_ARG && mentions("draw 1"), "build: negative draw field");
    }
    const soc_draw beyond_indices = make_draw(3, 10, 0, 30);   // 3 + 30 > 30
    const struct { const char* word; soc_draw bad; } shapes[] = {
        {"index_count", beyond_indices},
        {"vertex_count", make_draw(0, 10, 1, 30)},   // [1, 31) outside 30 vertices
        {"transform", make_draw(0, 10, 0, 30, 2)},
        {"material", make_draw(0, 10, 0, 30, 0, 2)}};
    for (const auto& c : shapes) {
        const std::vector<soc_draw> ds{ok, ok, c.bad};
        const soc_draw_scene sc = make_scene(ds);
        expect(soc_draw_scene_build(&sc, nullptr) == SOC_E_SHAPE && mentions("draw 2") && mentions(c.word) &&
                   mentions("soc_draw_scene_build"), "build: draw outside its arrays");
    }
    {
        const std::vector<soc_draw> ds{make_draw(0, 10, 0, 30, -1)};
        const soc_draw_scene sc = make_scene(ds);
        expect(soc_draw_scene_build(&sc, nullptr) == SOC_E_SHAPE && mentions("draw 0"), "build: negative transform");
        // 0xFFFFFFFE triangles or more (draws may share an index range): the visibility key cannot hold their ids
        const std::vector<soc_draw> huge(7, make_draw(0, 0x7FFFFFFF / 3, 0, 3));
        soc_draw_scene hs = make_scene(huge);
        hs.index_count = 0x7FFFFFFF;
        expect(soc_draw_scene_build(&hs, nullptr) == SOC_E_SHAPE && mentions("too many triangles"), "build: too many triangles");
    }
    // the per-frame entry points make the same checks, then refuse a workspace that was never built: no launch
    float vp[16] = {0};
    HostImg depth(64, 36, SOC_FMT_D32F, 4), a(64, 36, SOC_FMT_RGBA16F, 8);
    std::vector<uint64_t> vis(64 * 36);
    const soc_material* mats = reinterpret_cast<const soc_material*>(256);
    const std::vector<soc_draw> out_of_range{ok, ok, beyond_indices};
    const soc_draw_scene unbuilt = make_scene(one), bad_scene = make_scene(out_of_range);
    for (int call = 0; call < 3; ++call) {
        const char* name = call == 0 ? "soc_raster_visibility_draws" : call == 1 ? "soc_raster_depth_draws" : "soc_gbuffer_resolve_draws";
        auto run = [&](const soc_draw_scene* sc) {
            if (call == 0) return soc_raster_visibility_draws(sc, vp, 1, vis.data(), 64, 36, 1, nullptr);
            if (call == 1) return soc_raster_depth_draws(sc, vp, 2, 1.25f, 1.75f, depth.img, nullptr);
            return soc_gbuffer_resolve_draws(&g, sc, mats, 2, vis.data(), depth.img, a.img, a.img, a.img, a.img, nullptr);
        };
        expect(run(nullptr) == SOC_E_INVALID_ARG && mentions(name), "per-frame: null scene");
        expect(run(&bad_scene) == SOC_E_SHAPE && mentions(name) && mentions("draw 2"), "per-frame: draw outside its arrays");
        expect(run(&unbuilt) == SOC_E_INVALID_ARG && mentions(name) && mentions("not built"), "per-frame: never built");
    }
    soc_draw_scene no_normals = make_scene(one);
    no_normals.normals = nullptr;
    expect(soc_gbuffer_resolve_draws(&g, &no_normals, mats, 2, vis.data(), depth.img, a.img, a.img, a.img, a.img, nullptr) ==
               SOC_E_INVALID_ARG && mentions("normals"), "per-frame: resolve without normals");
    soc_draw_scene_release(nullptr);
    soc_draw_scene_release(&unbuilt);   // an unknown workspace: no-op

    // the alpha-mask twins (check_mask_table): every refusal of tests/test_alpha_mask_abi.py, all before any HIP call
    soc_mesh mesh;
    std::memset(&mesh, 0, sizeof mesh);
    mesh.positions = mesh.normals = mesh.uvs = reinterpret_cast<const float*>(256);
    mesh.indices = reinterpret_cast<const uint32_t*>(256);
    mesh.vertex_count = 3;
    mesh.triangle_count = 1;
    void* ws = reinterpret_cast<void*>(4096);
    for (int k = 0; k < 3; ++k) {
        soc_mesh m = mesh;
        if (k == 2) m.uvs = nullptr;
        const soc_material* table = k == 0 ? nullptr : mats;
        const int32_t count = k == 1 ? 0 : 2;
        const char* word = k == 2 ? "uvs" : "materials";
        expect(soc_raster_visibility_masked(&m, vp, 1, vis.data(), 64, 36, 1, ws, table, count, nullptr) == SOC_E_INVALID_ARG &&
                   mentions("soc_raster_visibility_masked") && mentions(word), "masked visibility: table or uvs");
        expect(soc_raster_depth_masked(&m, vp, 2, 1.25f, 1.75f, depth.img, ws, table, count, nullptr) == SOC_E_INVALID_ARG &&
                   mentions("soc_raster_depth_masked") && mentions(word), "masked depth: table or uvs");
        soc_draw_scene sc = make_scene(one);
        if (k == 2) sc.uvs = nullptr;
        expect(soc_raster_visibility_draws_masked(&sc, vp, 1, vis.data(), 64, 36, 1, table, count, nullptr) == SOC_E_INVALID_ARG &&
                   mentions("soc_raster_visibility_draws_masked") && mentions(word), "masked visibility of draws: table or uvs");
        expect(soc_raster_depth_draws_masked(&sc, vp, 2, 1.25f, 1.75f, depth.img, table, count, nullptr) == SOC_E_INVALID_ARG &&
                   mentions("soc_raster_depth_draws_masked") && mentions(word), "masked depth of draws: table or uvs");
    }
    expect(soc_raster_visibility_draws_masked(&unbuilt, vp, 1, vis.data(), 64, 36, 1, mats, 1, nullptr) == SOC_E_INVALID_ARG &&
               mentions("name up to 2"), "masked visibility of draws: fewer materials than the scene's");
    expect(soc_raster_depth_draws_masked(&unbuilt, vp, 2, 1.25f, 1.75f, depth.img, mats, 2, nullptr) == SOC_E_INVALID_ARG &&
               mentions("not built"), "masked depth of draws: never built");
    expect(soc_raster_visibility_draws_masked(nullptr, vp, 1, vis.data(), 64, 36, 1, mats, 2, nullptr) == SOC_E_INVALID_ARG,
           "masked visibility of draws: null scene");
    expect(soc_renderer_set_alpha_mask(nullptr, 1) == SOC_E_INVALID_ARG && mentions("soc_renderer_set_alpha_mask"),
           "set_alpha_mask: null renderer");
}
}  // namespace

int main() {
    soc_globals g;
    for (int pass = 0; pass < 2; ++pass) {
        const int W = pass ? 97 : 128, H = pass ? 55 : 72;   // even and odd extents
        globals_and_scene_feed(g, W, H);
        abi_introspection();
        render_graph(g, W, H);
        clouds_plan(g, W, H);
        composition_plan(g);
        post_plans(g);
        writers(W, H);
        oracle_frame(g, W, H);
        oracle_raster(g, W, H);
        draw_scenes(g);
    }
    for (float v : {0.0f, 1e-8f, 0.5f, 1.0f, 65504.0f, 1e9f, -3.0f, INFINITY, NAN})
        (void)soc_oracle_f16_to_f32(soc_oracle_f32_to_f16(v));
    for (float v : {0.0f, 1e-3f, 1.0f, 4096.0f, NAN, INFINITY}) (void)soc_oracle_luminance_bin(v, v, v, 12.77568f, -17.22432f);
    std::printf("san_host: %s (%d failed checks)\n", g_fail ? "FAILED" : "ok", g_fail);
    return g_fail ? 1 : 0;
}
