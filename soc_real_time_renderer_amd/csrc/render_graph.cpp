// render_graph.cpp — construction of the render graph (struct soc_renderer, renderer.hpp): the passes in the reference's
// add_task order, the caller's and the library-owned inserted passes, the dependencies and signals derived from the declared
// uses, and the entry points that create, destroy, configure and inspect a graph. Running a frame is render_execute.cpp.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "composition_plan.hpp"
#include "post_plan.hpp"
#include "renderer.hpp"

using namespace soc;

namespace {
using PassFn = soc_renderer::PassFn;

uint64_t res_mask(std::initializer_list<int> ids) {
    uint64_t m = 0;
    for (int i : ids) m |= 1ull << i;
    return m;
}

// SOC_RENDERER_VELOCITY_SLOTS: the frame's velocity image is the history_velocity slot the next frame reads as its
// previous velocity, so VELOCITY and PREVIOUS_VELOCITY name the two slots of one ping-pong pair; a use of either is
// taken as a use of both, which orders a next frame's velocity write after every reader of the slot it overwrites.
uint64_t widen_velocity(const soc_renderer* r, uint64_t m) {
    const uint64_t both = (1ull << SOC_RES_VELOCITY) | (1ull << SOC_RES_PREVIOUS_VELOCITY);
    return (r->flags & SOC_RENDERER_VELOCITY_SLOTS) && (m & both) ? m | both : m;
}

// The frame's velocity image: images.velocity, or with SOC_RENDERER_VELOCITY_SLOTS the history_velocity slot this frame
// resolves into (the reference copies velocity there after TAA, renderer.cpp:1185-1189; here its producer writes it there).
soc_img frame_velocity(const soc_renderer* r) {
    return (r->flags & SOC_RENDERER_VELOCITY_SLOTS) ? r->img.history_velocity[1 - r->hist] : r->img.velocity;
}

soc_renderer::Pass& add_pass(soc_renderer* r, std::string name, std::string group, int phase, uint64_t reads,
                             uint64_t writes, PassFn fn, uint32_t flags = 0) {
    soc_renderer::Pass p;
    p.name = std::move(name);
    p.group = std::move(group);
    p.phase = phase;
    p.reads = widen_velocity(r, reads);
    p.writes = widen_velocity(r, writes);
    p.flags = flags;
    p.run = std::move(fn);
    r->passes.push_back(std::move(p));
    return r->passes.back();
}

// Raster head of the graph (renderer.cpp:965-1021): depth prepass, sun shadow, G-buffer.
void build_raster_passes(soc_renderer* r) {
    if (!r->has_scene) return;
    const int pre = SOC_PHASE_PRE_EXPOSURE;
    // DepthPrepassTask writes depth (depth_prepass.inl); here the visibility buffer it becomes
    add_pass(r, "DepthPrepass", "Depth Prepass", pre, 0, res_mask({SOC_RES_VISIBILITY}),
             [r](const soc_globals* g, hipStream_t s) {
                 const soc_img& d = r->img.depth;
                 const float* pv = g->camera_projection_view_matrix;
                 const soc_raster_scene& sc = r->scene;
                 if (r->alpha_mask)   // soc_renderer_set_alpha_mask: the masked twins with the head's material table
                     return r->has_draws
                         ? soc_raster_visibility_draws_masked(&r->draw_scene, pv, SOC_CULL_FRONT, sc.visibility, d.width, d.height, 1,
                                                              sc.materials, sc.material_count, (soc_stream)s)
                         : soc_raster_visibility_masked(&sc.mesh, pv, SOC_CULL_FRONT, sc.visibility, d.width, d.height, 1,
                                                        sc.workspace, sc.materials, sc.material_count, (soc_stream)s);
                 if (r->has_draws)
                     return soc_raster_visibility_draws(&r->draw_scene, g->camera_projection_view_matrix, SOC_CULL_FRONT,
                                                        r->scene.visibility, d.width, d.height, 1, (soc_stream)s);
                 return soc_raster_visibility(&r->scene.mesh, g->camera_projection_view_matrix, SOC_CULL_FRONT,
                                              r->scene.visibility, d.width, d.height, 1, r->scene.workspace, (soc_stream)s);
             });
    // With its own workspace the shadow draw reads nothing the main lane writes in the frame: it runs on the second lane
    // beside the depth prepass and the G-buffer (SOC_RENDERER_SHADOW_LANE=0: on the main lane, in the shared workspace).
    // A draw scene's workspace holds the sun view's buffers itself.
    const bool shadow_lane = (r->has_draws || r->shadow_ws) && tuning_knob("SOC_RENDERER_SHADOW_LANE", 1);
    if (r->scene.shadow)
        add_pass(r, "SunShadowDraw", "Shadows", pre, 0, res_mask({SOC_RES_SUN_SHADOW}),
                 [r, shadow_lane](const soc_globals* g, hipStream_t s) {
                     // one shadow draw into `target` with the pipeline's cull and bias: the head's call, or with
                     // soc_renderer_set_alpha_mask its masked twin with the head's material table
                     auto draw = [r, shadow_lane, s](const float* pv, soc_img target) {
                         const soc_raster_scene& sc = r->scene;
                         void* ws = shadow_lane ? r->shadow_ws : sc.workspace;
                         if (r->alpha_mask)
                             return r->has_draws
                                 ? soc_raster_depth_draws_masked(&r->draw_scene, pv, SOC_CULL_BACK, 1.25f, 1.75f, target, sc.materials,
                                                                 sc.material_count, (soc_stream)s)
                                 : soc_raster_depth_masked(&sc.mesh, pv, SOC_CULL_BACK, 1.25f, 1.75f, target, ws, sc.materials,
                                                           sc.material_count, (soc_stream)s);
                         return r->has_draws ? soc_raster_depth_draws(&r->draw_scene, pv, SOC_CULL_BACK, 1.25f, 1.75f, target, (soc_stream)s)
                                             : soc_raster_depth(&sc.mesh, pv, SOC_CULL_BACK, 1.25f, 1.75f, target, ws, (soc_stream)s);
                     };
                     if (r->has_cascades) {   // every cascade into its slab of the atlas, same cull and bias
                         for (int k = 0; k < r->cascades.count; ++k) {
                             const int rc = draw(r->cascades.projection_view[k], r->cascade_slab(k));
                             if (rc) return rc;
                         }
                         return (int)SOC_OK;
                     }
                     return draw(g->sun_info.projection_view_matrix, r->img.shadow);
                 }, shadow_lane ? SOC_PASS_ASYNC : 0);
    // SunShadowDrawTerrainTask (renderer.cpp:983-990, sun_shadow_draw_terrain.inl): loads the shadow image SunShadowDraw
    // wrote and draws the terrain into it unbiased, on that pass's lane behind it (the layer's shadow workspace is its
    // own). A head without a shadow draw: the terrain's is the frame's only one, on the caller's stream, and clears.
    if (r->has_terrain && r->terrain.shadow) {
        const bool head_shadow = r->scene.shadow != 0;
        add_pass(r, "SunShadowDrawTerrain", "Shadows", pre, res_mask({SOC_RES_SUN_SHADOW}), res_mask({SOC_RES_SUN_SHADOW}),
                 [r, head_shadow](const soc_globals* g, hipStream_t s) {
                     if (r->has_cascades) {   // the terrain into every slab, unbiased, with the same clear rule
                         for (int k = 0; k < r->cascades.count; ++k) {
                             const int rc = soc_sun_shadow_draw_terrain(&r->terrain.shadow_mesh, r->cascades.projection_view[k],
                                                                        head_shadow ? 0 : 1, r->cascade_slab(k),
                                                                        r->terrain.shadow_workspace, (soc_stream)s);
                             if (rc) return rc;
                         }
                         return (int)SOC_OK;
                     }
                     return soc_sun_shadow_draw_terrain(&r->terrain.shadow_mesh, g->sun_info.projection_view_matrix,
                                                        head_shadow ? 0 : 1, r->img.shadow, r->terrain.shadow_workspace,
                                                        (soc_stream)s);
                 }, head_shadow && shadow_lane ? SOC_PASS_ASYNC : 0);
    }
    // GBufferGenerationTask uses (renderer.cpp:993-1005): albedo, emissive, normal, velocity, depth
    add_pass(r, "GBufferGeneration", "Rendering G-Buffer", pre, res_mask({SOC_RES_VISIBILITY}),
             res_mask({SOC_RES_ALBEDO, SOC_RES_EMISSIVE, SOC_RES_NORMAL, SOC_RES_VELOCITY, SOC_RES_DEPTH}),
             [r](const soc_globals* g, hipStream_t s) {
                 const soc_frame_images& I = r->img;
                 if (r->has_draws && r->motion_prev) {
                     // per-object motion vectors: the history array is kept here, on the caller's stream. A history that
                     // holds no frame yet is first made equal to the current transforms (the reference's velocity); after
                     // the resolve's vertex stage the current transforms become the next frame's history, ahead of the
                     // caller's next rewrite of them by stream order.
                     const soc_draw_scene& sc = r->draw_scene;
                     const size_t bytes = (size_t)sc.transform_count * sizeof(soc_transform);
                     const bool own = r->motion_prev != sc.transforms;   // the transforms as their own history: no copies
                     if (!r->motion_valid) {
                         if (own && hipMemcpyAsync(r->motion_prev, sc.transforms, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess)
                             return set_error(SOC_E_HIP, "GBufferGeneration: initialising the motion history failed");
                         r->motion_valid = true;
                     }
                     const int rc = soc_gbuffer_resolve_draws_motion(g, &sc, r->motion_prev, r->scene.materials,
                                                                     r->scene.material_count, r->scene.visibility, I.depth,
                                                                     I.albedo, I.emissive, I.normal, frame_velocity(r),
                                                                     (soc_stream)s);
                     if (rc) return rc;
                     if (own && hipMemcpyAsync(r->motion_prev, sc.transforms, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess)
                         return set_error(SOC_E_HIP, "GBufferGeneration: updating the motion history failed");
                     return SOC_OK;
                 }
                 if (r->has_draws)
                     return soc_gbuffer_resolve_draws(g, &r->draw_scene, r->scene.materials, r->scene.material_count,
                                                      r->scene.visibility, I.depth, I.albedo, I.emissive, I.normal,
                                                      frame_velocity(r), (soc_stream)s);
                 return soc_gbuffer_resolve(g, &r->scene.mesh, r->scene.materials, r->scene.material_count,
                                            r->scene.visibility, I.depth, I.albedo, I.emissive, I.normal,
                                            frame_velocity(r), r->scene.workspace, (soc_stream)s);
             });
    // DrawTerrainTask (renderer.cpp:1007-1021, draw_terrain.inl): loads the images GBufferGeneration wrote and depth-tests
    // the terrain into them (albedo, normal, velocity, depth; no emissive attachment). Its visibility buffer may be the
    // head's: GBufferGeneration has read that by then.
    if (r->has_terrain) {
        const uint64_t uses = res_mask({SOC_RES_VISIBILITY, SOC_RES_DEPTH, SOC_RES_ALBEDO, SOC_RES_NORMAL, SOC_RES_VELOCITY});
        add_pass(r, "DrawTerrain", "Rendering G-Buffer", pre, uses, uses, [r](const soc_globals* g, hipStream_t s) {
            const soc_frame_images& I = r->img;
            const soc_terrain_layer& t = r->terrain;
            return soc_draw_terrain(g, &t.mesh, t.materials, t.material_count, t.visibility, I.depth, I.albedo, I.normal,
                                    frame_velocity(r), t.workspace, (soc_stream)s);
        });
    }
}

// Bloom passes of the graph (renderer.cpp:1024-1062); build_passes_tail adds the rest.
void build_passes(soc_renderer* r) {
    auto& I = r->img;
    const int pre = SOC_PHASE_PRE_EXPOSURE;
    const int nm = 4;
    const soc_img& bloom_dst = r->bloom_image();
    const int dst_res = r->bloom_resource();
    const int mip[4] = {SOC_RES_BLOOM_MIP0, SOC_RES_BLOOM_MIP1, SOC_RES_BLOOM_MIP2, SOC_RES_BLOOM_MIP3};
    const bool chain_ok = bloom_fused_applicable(I.emissive, I.bloom_mips, nm, bloom_dst);
    r->bloom_in_comp = false;
    if (chain_ok && !(r->flags & (SOC_RENDERER_EXACT_BLOOM | SOC_RENDERER_UNFUSED_BLOOM))) {
        // weighted form (bloom_w.hip): 4 launches, mip0 / mip2 only in LDS, within the RGBA16F tolerance
        static const char* names[4] = {"BloomDownsample - 0+1", "BloomDownsample - 2+3", "BloomUpsample - 3+2",
                                       "BloomUpsample - 1+0"};
        const uint64_t rd[4] = {res_mask({SOC_RES_EMISSIVE}), res_mask({mip[1]}), res_mask({mip[3]}), res_mask({mip[1]})};
        const uint64_t wr[4] = {res_mask({mip[1]}), res_mask({mip[3]}), res_mask({mip[1]}), res_mask({dst_res})};
        // SOC_RENDERER_BLOOM_IN_COMPOSITION: where the fused composition + histogram's pair path applies, the last stage
        // (mip1 -> [mip0] -> output) may run inside that launch (composition_pair<..., BL>) in a frame whose sky lane is
        // the critical path (high priority, bloom_in_comp_active): the fourth pass then records nothing and the bloom
        // output is not written. Beside a low-priority sky lane the fused kernel's 19 KiB of LDS per workgroup do not fit next to
        // the sun-visibility march's noise tables (C3: Composition 76 -> 122 us in the frame, -0.6 % fps; C4 +2.9 %,
        // profiles/r05_ab_bloom_in_composition.txt), so those frames keep the separate pass.
        soc_globals gres{};
        gres.resolution[0] = I.color.width;
        gres.resolution[1] = I.color.height;
        r->bloom_in_comp = (r->flags & SOC_RENDERER_BLOOM_IN_COMPOSITION) && !(r->flags & SOC_RENDERER_UNFUSED_HISTOGRAM) &&
                           soc::composition_pair_applicable(&gres, I.color, I.albedo, bloom_dst, I.normal, I.depth, I.clouds);
        for (int st = 1; st <= 4; ++st)
            add_pass(r, names[st - 1], "Bloom", pre, rd[st - 1], wr[st - 1], [r, st](const soc_globals* g, hipStream_t s) {
                if (st == 4 && bloom_in_comp_active(r)) return (int)SOC_OK;   // Composition computes it this frame
                const soc_img& dst = r->bloom_image();
                // SOC_BLOOM_SPARSE: strips proven zero from mip3 are left unwritten; Composition proves the same cells
                if (st == 4 && r->bloom_sparse_frame)
                    return soc::bloom_weighted(r->img.emissive, r->img.bloom_mips, dst, s, 4, true);
                return soc_bloom_weighted_stage(g, r->img.emissive, r->img.bloom_mips, 4, dst, st, (soc_stream)s);
            });
        return;
    }
    // renderer.cpp:1024-1042: the bit-exact per-pass chain (SOC_RENDERER_EXACT_BLOOM / _UNFUSED_BLOOM, or mips that do
    // not halve exactly)
    add_pass(r, "BloomDownsample - 0", "Bloom", pre, res_mask({SOC_RES_EMISSIVE}), res_mask({mip[0]}),
             [r](const soc_globals* g, hipStream_t s) {
                 return soc_bloom_downsample(g, r->img.emissive, r->img.bloom_mips[0], (soc_stream)s);
             });
    for (int i = 0; i < nm - 1; ++i)
        add_pass(r, "BloomDownsample - " + std::to_string(i + 1), "Bloom", pre, res_mask({mip[i]}),
                 res_mask({mip[i + 1]}), [r, i](const soc_globals* g, hipStream_t s) {
                     return soc_bloom_downsample(g, r->img.bloom_mips[i], r->img.bloom_mips[i + 1], (soc_stream)s);
                 });
    // renderer.cpp:1044-1062 (load_op CLEAR: the upsample overwrites its target, quirk Q5)
    for (int i = nm - 1; i > 0; --i)
        add_pass(r, "BloomUpsample - " + std::to_string(i), "Bloom", pre, res_mask({mip[i]}), res_mask({mip[i - 1]}),
                 [r, i](const soc_globals* g, hipStream_t s) {
                     return soc_bloom_upsample(g, r->img.bloom_mips[i], r->img.bloom_mips[i - 1], (soc_stream)s);
                 });
    add_pass(r, "BloomUpsample - 0", "Bloom", pre, res_mask({mip[0]}), res_mask({dst_res}),
             [r](const soc_globals* g, hipStream_t s) {
                 return soc_bloom_upsample(g, r->img.bloom_mips[0], r->bloom_image(), (soc_stream)s);
             });
}

// the frame's Composition call: the globals and the images (the bloom output is the emissive input)
soc::CompositionCall composition_call(const soc_renderer* r, const soc_globals* g) {
    const auto& I = r->img;
    return soc::composition_call(g, I.d_globals,
                                 {I.color, I.albedo, r->bloom_image(), I.normal, I.depth, I.ssao_blur, I.shadow, I.clouds});
}

void build_passes_tail(soc_renderer* r) {
    auto& I = r->img;
    const int pre = SOC_PHASE_PRE_EXPOSURE, post = SOC_PHASE_POST_EXPOSURE;
    const int em_res = r->bloom_resource();
    // renderer.cpp:1064-1079
    add_pass(r, "SSAOGeneration", "Ambient Occlusion", pre, res_mask({SOC_RES_DEPTH, SOC_RES_NORMAL}),
             res_mask({SOC_RES_SSAO}), [r](const soc_globals* g, hipStream_t s) {
                 return soc_ssao_generation(g, r->img.depth, r->img.normal, r->img.ssao, r->img.ssao_noise_table,
                                            (soc_stream)s);
             });
    add_pass(r, "SSAOBlur", "Ambient Occlusion", pre, res_mask({SOC_RES_SSAO}), res_mask({SOC_RES_SSAO_BLUR}),
             [r](const soc_globals* g, hipStream_t s) { return soc_ssao_blur(g, r->img.ssao, r->img.ssao_blur, (soc_stream)s); });
    // Sky split: with the fused histogram on the pair path, the clouds lane also writes and bins the colour
    // image's sky pixels (sky_compose_launch), and Composition skips them, so it does not wait for the clouds.
    const bool fused_hist = !(r->flags & SOC_RENDERER_UNFUSED_HISTOGRAM);
    soc_globals gres{};
    gres.resolution[0] = I.color.width;
    gres.resolution[1] = I.color.height;
    r->sky_split = fused_hist && !(r->flags & SOC_RENDERER_NO_SKY_SPLIT) &&
                   soc::composition_pair_applicable(&gres, I.color, I.albedo, r->bloom_image(), I.normal, I.depth, I.clouds);
    const uint64_t sky_w = r->sky_split ? res_mask({SOC_RES_SKY_COLOR, SOC_RES_SKY_HISTOGRAM_PARTIALS}) : 0;
    const uint64_t parts = res_mask({SOC_RES_HISTOGRAM_PARTIALS}) | (r->sky_split ? res_mask({SOC_RES_SKY_HISTOGRAM_PARTIALS}) : 0);
    // renderer.cpp:1094-1101. Under the sky split the second lane then writes and bins the colour's sky pixels
    // (SkyCompose, composition.inl:220-222): a pass of its own, so CloudRendering itself has no cross-lane ring edge
    // (it writes only CLOUDS) and, with SOC_RENDERER_STATIC_INPUTS, may start before the fork.
    add_pass(r, "CloudRendering", "Sky Rendering", pre, res_mask({SOC_RES_DEPTH, SOC_RES_NOISE}), res_mask({SOC_RES_CLOUDS}),
             [r](const soc_globals* g, hipStream_t s) {
                 // a sky lane at high priority (the lane probe found the frame sky-bound): the density grid at twice
                 // the resident set (C4 +2.7 %, C3 -0.8 %: profiles/r05_ab_clouds_density_mult.txt) and the hoisted
                 // classification (C4 +1.8 %, C3 -1.1 %); else the knobs
                 // (also during the lane probe's high-priority windows, so the probe compares the two alternatives
                 // as they run: high with these variants against low without)
                 const bool sky_bound = sky_lane_high(r) && tuning_knob("SOC_RENDERER_SKY_BOUND_VARIANTS", 1);
                 return soc::cloud_rendering_launch(g, r->img.depth, r->img.noise, r->img.clouds, r->img.clouds_workspace,
                                                    (soc_stream)s, sky_bound, &r->clouds_state);
             }, SOC_PASS_ASYNC);
    if (r->sky_split)
        add_pass(r, "SkyCompose", "Sky Rendering", pre, res_mask({SOC_RES_CLOUDS, SOC_RES_DEPTH}), sky_w,
                 [r](const soc_globals* g, hipStream_t s) {
                     return soc::sky_compose_launch(g, r->img.color, r->img.depth, r->img.clouds, r->hist_scratch,
                                                    (soc_stream)s);
                 }, SOC_PASS_ASYNC);
    // renderer.cpp:1103-1117 (composition uses) and 1155-1162 (histogram): one launch by default (the colour
    // is binned as it is written), two with SOC_RENDERER_UNFUSED_HISTOGRAM (measured in composition.hip)
    const uint64_t comp_reads = res_mask({SOC_RES_ALBEDO, em_res, SOC_RES_NORMAL, SOC_RES_DEPTH, SOC_RES_SSAO_BLUR,
                                          SOC_RES_SUN_SHADOW}) | (r->bloom_in_comp ? res_mask({SOC_RES_BLOOM_MIP1, SOC_RES_BLOOM_MIP3}) : 0) |
                                (r->sky_split ? 0 : res_mask({SOC_RES_CLOUDS}));
    if (fused_hist) {
        add_pass(r, "Composition+GenerateLuminanceHistogram", "Composition", pre, comp_reads,
                 res_mask({SOC_RES_COLOR, SOC_RES_HISTOGRAM_PARTIALS}), [r](const soc_globals* g, hipStream_t s) {
                     const soc::LightBoundsCall lb = {r->light_bounds, r->light_flags, nullptr};
                     soc::CompositionCall c = composition_call(r, g);
                     c.histogram = true;
                     c.ae = r->img.auto_exposure;
                     c.scratch = r->hist_scratch;
                     c.sky_external = r->sky_split_active;
                     c.bloom_mip1 = bloom_in_comp_active(r) ? &r->img.bloom_mips[1] : nullptr;
                     c.bloom_mip3 = r->bloom_cells_frame ? &r->img.bloom_mips[3] : nullptr;
                     c.bounds = r->light_bounds ? &lb : nullptr;
                     c.cascades = r->has_cascades ? &r->cascades : nullptr;
                     c.cascaded = r->has_cascades;
                     return soc::composition(c, (soc_stream)s);
                 });
        // the 8 partial histograms of the fused launch into the AutoExposure bins. Before a multi-GPU exchange
        // (PRE and POST in separate calls) the fold must precede it; in a one-call frame the resolve folds them
        // itself and this pass has no work (it is then neither launched nor timed).
        auto& fold = add_pass(r, "LuminanceHistogramFold", "Auto Exposure", pre, parts,
                              res_mask({SOC_RES_AUTO_EXPOSURE}) | parts,
                              [r](const soc_globals* g, hipStream_t s) {
                                  (void)g;
                                  return soc::histogram_fold_launch(r->hist_scratch, r->img.auto_exposure, (soc_stream)s);
                              });
        fold.skip = [r] { return r->fold_in_resolve; };
    } else {
        add_pass(r, "Composition", "Composition", pre, comp_reads, res_mask({SOC_RES_COLOR}),
                 [r](const soc_globals* g, hipStream_t s) {
                     // the cascades come without bounded lights (soc_composition_cascaded, else soc_composition_bounded)
                     const soc::LightBoundsCall lb = {r->light_bounds, r->light_flags, nullptr};
                     soc::CompositionCall c = composition_call(r, g);
                     c.bounds = r->light_bounds && !r->has_cascades ? &lb : nullptr;
                     c.cascades = r->has_cascades ? &r->cascades : nullptr;
                     c.cascaded = r->has_cascades;
                     return soc::composition(c, (soc_stream)s);
                 });
        add_pass(r, "GenerateLuminanceHistogram", "Auto Exposure", pre, res_mask({SOC_RES_COLOR}),
                 res_mask({SOC_RES_AUTO_EXPOSURE}), [r](const soc_globals* g, hipStream_t s) {
                     return soc_generate_luminance_histogram(g, r->img.color, r->img.auto_exposure, (soc_stream)s);
                 });
    }
    // renderer.cpp:1164-1168
    add_pass(r, "ResolveLuminanceHistogram", "Auto Exposure", post, res_mask({SOC_RES_AUTO_EXPOSURE}) | parts,
             res_mask({SOC_RES_AUTO_EXPOSURE}) | parts, [r](const soc_globals* g, hipStream_t s) {
                 return soc::resolve_luminance_histogram(g, r->img.auto_exposure, r->total_pixels, r->wide,
                                                         r->fold_in_resolve ? r->hist_scratch : nullptr, (soc_stream)s);
             });
    // renderer.cpp:1170-1198: TAA + both history copies (ping-pong + fused velocity history; with
    // SOC_RENDERER_VELOCITY_SLOTS the velocity is already in its history slot: no copy), and
    // renderer.cpp:1210-1217: tone mapping, fused into the TAA launch for an RGBA8 (UNORM or SRGB) framebuffer
    const bool vslots = r->flags & SOC_RENDERER_VELOCITY_SLOTS;
    const uint64_t taa_reads = res_mask({SOC_RES_COLOR, SOC_RES_PREVIOUS_COLOR, SOC_RES_VELOCITY,
                                         SOC_RES_PREVIOUS_VELOCITY, SOC_RES_DEPTH}) |
                               (r->sky_split ? res_mask({SOC_RES_SKY_COLOR}) : 0);
    const uint64_t taa_writes = vslots ? res_mask({SOC_RES_RESOLVED}) : res_mask({SOC_RES_RESOLVED, SOC_RES_PREVIOUS_VELOCITY});
    const bool fuse_tm = !(r->flags & SOC_RENDERER_UNFUSED_TONEMAP) &&
                         (I.output.format == SOC_FMT_RGBA8_UNORM || I.output.format == SOC_FMT_RGBA8_SRGB);
    if (fuse_tm) {
        add_pass(r, "TemporalAntiAliasing+ToneMapping", "Temporal Anti-Aliasing", post,
                 taa_reads | res_mask({SOC_RES_AUTO_EXPOSURE}), taa_writes | res_mask({SOC_RES_OUTPUT}),
                 [r](const soc_globals* g, hipStream_t s) {
                     const auto& I = r->img;
                     const int p = r->hist, q = 1 - r->hist;
                     const bool slots = r->flags & SOC_RENDERER_VELOCITY_SLOTS;
                     return soc_temporal_antialiasing_tone_mapping(g, I.history_color[q], I.color, I.history_color[p],
                                                                   frame_velocity(r), I.history_velocity[p], I.depth,
                                                                   slots ? soc_img{} : I.history_velocity[q],
                                                                   I.auto_exposure, I.output, (soc_stream)s);
                 });
    } else {
        add_pass(r, "TemporalAntiAliasing", "Temporal Anti-Aliasing", post, taa_reads, taa_writes,
                 [r](const soc_globals* g, hipStream_t s) {
                     const auto& I = r->img;
                     const int p = r->hist, q = 1 - r->hist;
                     const bool slots = r->flags & SOC_RENDERER_VELOCITY_SLOTS;
                     return soc_temporal_antialiasing(g, I.history_color[q], I.color, I.history_color[p],
                                                      frame_velocity(r), I.history_velocity[p], I.depth,
                                                      slots ? soc_img{} : I.history_velocity[q], (soc_stream)s);
                 });
        add_pass(r, "ToneMapping", "Tone Mapping", post, res_mask({SOC_RES_RESOLVED, SOC_RES_AUTO_EXPOSURE}),
                 res_mask({SOC_RES_OUTPUT}), [r](const soc_globals* g, hipStream_t s) {
                     const auto& I = r->img;
                     return soc_tone_mapping(g, I.history_color[1 - r->hist], I.auto_exposure, I.output, (soc_stream)s);
                 });
    }
}

// The frame as a caller pass sees it: history slot 0 = PREVIOUS, 1 = RESOLVED of this frame.
soc_frame_images callback_view(const soc_renderer* r) {
    soc_frame_images v = r->img;
    const int p = r->hist, q = 1 - r->hist;
    v.history_color[0] = r->img.history_color[p];
    v.history_color[1] = r->img.history_color[q];
    v.history_velocity[0] = r->img.history_velocity[p];
    v.history_velocity[1] = r->img.history_velocity[q];
    v.velocity = frame_velocity(r);
    return v;
}

uint64_t desc_mask(const int32_t* ids, int32_t n) {
    uint64_t m = 0;
    for (int i = 0; i < n; ++i) m |= 1ull << ids[i];
    return m;
}

// Under the sky split COLOR is the non-sky pixels and SKY_COLOR the sky pixels of the same image (and the partial
// histograms have a sky copy): a caller pass declaring COLOR (or the partials) gets both, so it is ordered against
// the second lane's sky writes too.
uint64_t widen_sky(const soc_renderer* r, uint64_t m) {
    if (!r->sky_split) return m;
    if (m & (1ull << SOC_RES_COLOR)) m |= 1ull << SOC_RES_SKY_COLOR;
    if (m & (1ull << SOC_RES_HISTOGRAM_PARTIALS)) m |= 1ull << SOC_RES_SKY_HISTOGRAM_PARTIALS;
    return m;
}

// Insert the caller passes: before their anchor, or at the end of their phase. Returns an error for an
// unknown or cross-phase anchor.
int insert_user_passes(soc_renderer* r) {
    for (auto& up : r->user_passes) {
        soc_renderer::Pass p;
        p.name = up.name;
        p.group = up.group;
        p.phase = up.desc.phase;
        p.reads = widen_velocity(r, widen_sky(r, desc_mask(up.desc.reads, up.desc.read_count)));
        p.writes = widen_velocity(r, widen_sky(r, desc_mask(up.desc.writes, up.desc.write_count)));
        p.flags = up.desc.flags;
        p.run = up.run;
        size_t at = r->passes.size();
        if (!up.before.empty()) {
            at = r->passes.size() + 1;
            for (size_t i = 0; i < r->passes.size(); ++i)
                if (up.before_prefix ? r->passes[i].name.compare(0, up.before.size(), up.before) == 0
                                     : r->passes[i].name == up.before) { at = i; break; }
            if (at > r->passes.size())
                return set_error(SOC_E_INVALID_ARG, "soc_renderer_add_pass: no pass named \"%s\"", up.before.c_str());
            if (r->passes[at].phase != p.phase)
                return set_error(SOC_E_INVALID_ARG, "soc_renderer_add_pass: \"%s\" is in another phase", up.before.c_str());
        } else {
            for (size_t i = 0; i < r->passes.size(); ++i)
                if (r->passes[i].phase > p.phase) { at = i; break; }
        }
        r->passes.insert(r->passes.begin() + (long)at, std::move(p));
    }
    return SOC_OK;
}

// Dependencies from the declared uses: for every resource a pass reads, the latest earlier writer (RAW);
// for every resource it writes, the latest earlier writer (WAW) and the readers since then (WAR).
//
// Cross-frame (ring) edges: the graph runs frame after frame, so the pass list is a ring. For a resource that no
// earlier pass of its own frame writes, the walk goes on into the PREVIOUS frame, from the last pass back to the
// pass itself: the latest writer there (RAW / WAW) and, for a write, the readers since that writer (WAR). The TAA
// history pair swaps each frame (ping-pong: this frame's PREVIOUS_COLOR is the last frame's RESOLVED), so in the
// previous frame the walk looks at the swapped resource. Example: GBufferGeneration writes DEPTH, which the
// previous frame's CloudRendering (second lane) still reads: a WAR ring edge across the lanes.
int prev_frame_resource(int b) {
    if (b == SOC_RES_PREVIOUS_COLOR) return SOC_RES_RESOLVED;
    if (b == SOC_RES_RESOLVED) return SOC_RES_PREVIOUS_COLOR;
    return b;
}

void derive_dependencies(soc_renderer* r) {
    const int n = (int)r->passes.size();
    for (int i = 0; i < n; ++i) {
        auto& p = r->passes[i];
        p.deps.clear();
        p.carry.clear();
        std::vector<char> dep(n, 0), carry(n, 0);
        for (int b = 0; b < SOC_RES_COUNT; ++b) {
            const uint64_t bit = 1ull << b;
            if (!((p.reads | p.writes) & bit)) continue;
            bool writer = false;
            for (int j = i - 1; j >= 0 && !writer; --j) {
                const auto& q = r->passes[j];
                if (q.writes & bit) { dep[j] = 1; writer = true; }       // RAW / WAW: the latest writer
                else if ((p.writes & bit) && (q.reads & bit)) dep[j] = 1; // WAR: readers since that writer
            }
            if (writer) continue;
            const uint64_t pbit = 1ull << prev_frame_resource(b);
            for (int j = n - 1; j >= i; --j) {                           // the previous frame, back to pass i itself
                const auto& q = r->passes[j];
                if (q.writes & pbit) { carry[j] = 1; break; }
                if ((p.writes & bit) && (q.reads & pbit)) carry[j] = 1;
            }
        }
        for (int j = 0; j < n; ++j) {
            if (dep[j]) p.deps.push_back(j);
            if (carry[j]) p.carry.push_back(j);
        }
    }
}

// A pass records its completion event when a pass of the other lane may wait on it: an in-frame dependency across
// the lanes, or a ring edge from a main-lane pass onto a second-lane pass (waited on only when the previous call ended
// without its join). Ring edges from second-lane passes onto main-lane passes are covered by the fork, so a main-lane
// pass whose only cross-lane dependents are such edges records nothing (an event record costs its queue a marker).
void derive_signals(soc_renderer* r) {
    const int n = (int)r->passes.size();
    for (auto& p : r->passes) p.signal = false;
    for (int i = 0; i < n; ++i) {
        const bool li = (r->passes[i].flags & SOC_PASS_ASYNC) != 0;
        for (int j : r->passes[i].deps)
            if (((r->passes[j].flags & SOC_PASS_ASYNC) != 0) != li) r->passes[j].signal = true;
        if (!li)
            for (int j : r->passes[i].carry)
                if ((r->passes[j].flags & SOC_PASS_ASYNC) != 0) r->passes[j].signal = true;
    }
}

int build_graph(soc_renderer* r) {
    r->inputs_ordered = false;
    destroy_pass_events(r);
    r->passes.clear();
    build_raster_passes(r);
    build_passes(r);
    build_passes_tail(r);
    int rc = insert_user_passes(r);
    // SOC_BLOOM_SPARSE needs a graph in which nobody but Composition reads the bloom output (a caller's pass that
    // declares it, or the in-place output that is the emissive image, gets every pixel written)
    r->bloom_sparse = r->bloom_in_comp && r->img.bloom_output.data;
    for (const auto& p : r->passes) {
        const uint64_t bo = 1ull << SOC_RES_BLOOM_OUTPUT;
        if ((p.reads & bo) && p.name != "Composition+GenerateLuminanceHistogram") r->bloom_sparse = false;
        if ((p.writes & bo) && p.name != "BloomUpsample - 1+0") r->bloom_sparse = false;
    }
    derive_dependencies(r);
    derive_signals(r);
    return rc;
}

// build_graph, and the pass timing of a SOC_RENDERER_TIMING renderer on again for the new passes.
int rebuild(soc_renderer* r) {
    const int rc = build_graph(r);
    if (rc) return rc;
    return (r->flags & SOC_RENDERER_TIMING) ? soc_renderer_set_pass_timing(r, -1, 1) : (int)SOC_OK;
}
}  // namespace

void soc::destroy_pass_events(soc_renderer* r) {
    for (auto& p : r->passes) {
        for (auto e : p.ev0) (void)hipEventDestroy(e);
        for (auto e : p.ev1) (void)hipEventDestroy(e);
        if (p.done) (void)hipEventDestroy(p.done);
    }
}

extern "C" soc_renderer* soc_renderer_create(const soc_frame_images* images, uint32_t flags) {
    if (!images) {
        set_error(SOC_E_INVALID_ARG, "soc_renderer_create: null images");
        return nullptr;
    }
    if (!images->auto_exposure) {
        set_error(SOC_E_INVALID_ARG, "soc_renderer_create: auto_exposure buffer required");
        return nullptr;
    }
    if ((flags & SOC_RENDERER_VELOCITY_SLOTS) &&
        (!images->history_velocity[0].data || !images->history_velocity[1].data ||
         images->history_velocity[0].data == images->history_velocity[1].data)) {
        set_error(SOC_E_INVALID_ARG, "soc_renderer_create: SOC_RENDERER_VELOCITY_SLOTS needs two distinct history_velocity images");
        return nullptr;
    }
    soc_renderer* r = new soc_renderer();
    r->img = *images;
    r->flags = flags;
    r->async = !(flags & SOC_RENDERER_SERIAL);
    if (rebuild(r) != SOC_OK) {
        soc_renderer_destroy(r);
        return nullptr;
    }
    return r;
}

extern "C" void soc_renderer_destroy(soc_renderer* r) {
    if (!r) return;
    destroy_pass_events(r);
    for (auto& e : r->staging_ev)
        if (e) (void)hipEventDestroy(e);
    if (r->staging) (void)hipHostFree(r->staging);
    destroy_side_lane(r);
    if (r->hist_scratch) (void)hipFree(r->hist_scratch);
    if (r->shadow_ws) (void)hipFree(r->shadow_ws);
    delete r;
}

// The sun shadow draw's own workspace (SOC_RENDERER_SHADOW_LANE). Tuning knob SOC_TEST_FAIL_SHADOW_WS=1 injects the
// allocation failure for the tests (a real hipMalloc that fails, so HIP's last error is set as by a true OOM).
static hipError_t shadow_ws_alloc(void** p, size_t n) {
    if (tuning_knob("SOC_TEST_FAIL_SHADOW_WS", 0)) return hipMalloc(p, (size_t)1 << 62);
    return hipMalloc(p, n);
}

extern "C" int soc_renderer_set_raster_scene(soc_renderer* r, const soc_raster_scene* scene) {
    if (!r) return set_error(SOC_E_INVALID_ARG, "soc_renderer_set_raster_scene: null renderer");
    if (scene) {
        if (!scene->materials || scene->material_count <= 0 || !scene->visibility || !scene->workspace ||
            !scene->mesh.positions || !scene->mesh.normals || !scene->mesh.uvs || !scene->mesh.indices)
            return set_error(SOC_E_INVALID_ARG, "soc_renderer_set_raster_scene: incomplete scene");
        if (scene->shadow && !r->img.shadow.data)
            return set_error(SOC_E_INVALID_ARG, "soc_renderer_set_raster_scene: shadow pass needs images.shadow");
    }
    if (scene && scene->shadow) {
        const size_t need = soc_raster_workspace_size(scene->mesh.vertex_count, scene->mesh.triangle_count);
        if (need > r->shadow_ws_bytes) {
            if (r->shadow_ws) (void)hipFree(r->shadow_ws);
            r->shadow_ws = nullptr;
            r->shadow_ws_bytes = 0;
            // on failure: the shared workspace; clear HIP's sticky last error so the next pass's check_launch() does
            // not report this allocation's out-of-memory as a launch failure
            if (shadow_ws_alloc(&r->shadow_ws, need) != hipSuccess) {
                r->shadow_ws = nullptr;
                (void)hipGetLastError();
            } else {
                r->shadow_ws_bytes = need;
            }
        }
    }
    r->has_scene = scene != nullptr;
    if (!scene) r->has_terrain = false;   // the terrain layer goes with the head it is drawn over
    r->has_draws = false;
    r->draws.clear();
    r->motion_prev = nullptr;   // a new scene turns per-object motion off (soc_renderer_set_draw_motion)
    r->motion_valid = false;
    if (scene) r->scene = *scene;
    return rebuild(r);
}

extern "C" int soc_renderer_set_draw_scene(soc_renderer* r, const soc_draw_scene* scene, const soc_material* d_materials,
                                           int32_t material_count, int32_t shadow, uint64_t* visibility) {
    if (!r) return set_error(SOC_E_INVALID_ARG, "soc_renderer_set_draw_scene: null renderer");
    if (!scene) return soc_renderer_set_raster_scene(r, nullptr);
    if (!d_materials || material_count <= 0 || !visibility || !scene->positions || !scene->normals || !scene->uvs ||
        !scene->indices || !scene->transforms || !scene->workspace || scene->draw_count < 0 ||
        (scene->draw_count > 0 && !scene->draws))
        return set_error(SOC_E_INVALID_ARG, "soc_renderer_set_draw_scene: incomplete scene");
    if (material_count < scene->material_count)
        return set_error(SOC_E_SHAPE, "soc_renderer_set_draw_scene: %d materials, the scene's draws name up to %d", material_count,
                         scene->material_count);
    if (shadow && !r->img.shadow.data)
        return set_error(SOC_E_INVALID_ARG, "soc_renderer_set_draw_scene: shadow pass needs images.shadow");
    // the draws' own checks (ranges, the build's outcome) are the *_draws entry points', every frame: a scene rebuilt or
    // never built is refused there, before any launch
    r->draws.assign(scene->draws, scene->draws + scene->draw_count);
    r->draw_scene = *scene;
    r->draw_scene.draws = r->draws.data();
    r->scene = soc_raster_scene{};
    r->scene.materials = d_materials;
    r->scene.material_count = material_count;
    r->scene.shadow = shadow != 0;
    r->scene.visibility = visibility;
    r->has_scene = r->has_draws = true;
    r->motion_prev = nullptr;   // the new scene may have another transform count: motion is set again after it
    r->motion_valid = false;
    return rebuild(r);
}

extern "C" int soc_renderer_set_draw_motion(soc_renderer* r, soc_transform* previous_transforms) {
    if (!r) return set_error(SOC_E_INVALID_ARG, "soc_renderer_set_draw_motion: null renderer");
    if (!r->has_draws) return set_error(SOC_E_INVALID_ARG, "soc_renderer_set_draw_motion: no draw scene is set");
    // the graph is not rebuilt: GBufferGeneration looks at motion_prev when it runs
    r->motion_prev = previous_transforms;
    r->motion_valid = false;
    return SOC_OK;
}

extern "C" int soc_renderer_set_terrain(soc_renderer* r, const soc_terrain_layer* layer) {
    const char* name = "soc_renderer_set_terrain";
    if (!r) return set_error(SOC_E_INVALID_ARG, "%s: null renderer", name);
    if (layer) {
        if (!r->has_scene)
            return set_error(SOC_E_INVALID_ARG, "%s: no raster head is set (soc_renderer_set_raster_scene / _set_draw_scene)", name);
        const soc_mesh& m = layer->mesh;
        if (!layer->materials || layer->material_count <= 0 || !layer->visibility || !layer->workspace || !m.positions ||
            !m.normals || !m.uvs || !m.indices || m.vertex_count < 0 || m.triangle_count < 0)
            return set_error(SOC_E_INVALID_ARG, "%s: incomplete layer (mesh arrays, materials, visibility, workspace)", name);
        if (layer->shadow) {
            if (!r->img.shadow.data) return set_error(SOC_E_INVALID_ARG, "%s: shadow pass needs images.shadow", name);
            if (!layer->shadow_workspace)
                return set_error(SOC_E_INVALID_ARG, "%s: shadow = 1 needs a shadow_workspace (of the shadow mesh)", name);
            const soc_mesh& sm = layer->shadow_mesh;
            if (sm.positions && (!sm.indices || sm.vertex_count < 0 || sm.triangle_count < 0))
                return set_error(SOC_E_INVALID_ARG, "%s: incomplete shadow_mesh (indices, counts)", name);
        }
        r->terrain = *layer;
        if (!layer->shadow_mesh.positions) r->terrain.shadow_mesh = layer->mesh;
    }
    r->has_terrain = layer != nullptr;
    const int rc = rebuild(r);
    if (rc) {   // a caller's pass could not be placed beside the new passes: the graph without the layer
        r->has_terrain = false;
        (void)rebuild(r);
    }
    return rc;
}

// Test hook (not in the public header): 1 when per-object motion is on, so its switching can be checked without a GPU.
extern "C" int soc_debug_draw_motion(const soc_renderer* r) { return r && r->has_draws && r->motion_prev ? 1 : 0; }

// Takes the last inserted pass out again and rebuilds the graph without it.
static void drop_last_user_pass(soc_renderer* r) {
    r->user_passes.pop_back();
    (void)rebuild(r);
}

// Registers the callable `run` under the descriptor `d`: the descriptor checks, the rebuild and the roll-back shared by
// soc_renderer_add_pass and the library-owned passes.
static int register_user_pass(soc_renderer* r, const soc_pass_desc* d, PassFn run, const char* before,
                              bool before_prefix = false) {
    if (d->phase != SOC_PHASE_PRE_EXPOSURE && d->phase != SOC_PHASE_POST_EXPOSURE)
        return set_error(SOC_E_INVALID_ARG, "soc_renderer_add_pass: %s: phase must be PRE or POST", d->name);
    if (d->read_count < 0 || d->read_count > SOC_PASS_MAX_USES || d->write_count < 0 || d->write_count > SOC_PASS_MAX_USES)
        return set_error(SOC_E_INVALID_ARG, "soc_renderer_add_pass: %s: at most %d reads / writes", d->name, SOC_PASS_MAX_USES);
    for (int i = 0; i < d->read_count + d->write_count; ++i) {
        const int id = i < d->read_count ? d->reads[i] : d->writes[i - d->read_count];
        if (id < 0 || id >= SOC_RES_COUNT)
            return set_error(SOC_E_INVALID_ARG, "soc_renderer_add_pass: %s: bad resource id %d", d->name, id);
    }
    for (const auto& p : r->passes)
        if (p.name == d->name) return set_error(SOC_E_INVALID_ARG, "soc_renderer_add_pass: duplicate pass name \"%s\"", d->name);
    soc_renderer::UserPass up;
    up.desc = *d;
    up.name = d->name;
    up.group = d->group ? d->group : "";
    up.before = before ? before : "";
    up.before_prefix = before_prefix;
    up.run = std::move(run);
    up.desc.name = nullptr;
    up.desc.group = nullptr;
    r->user_passes.push_back(std::move(up));
    const int rc = rebuild(r);
    if (rc) drop_last_user_pass(r);
    return rc;
}

extern "C" int soc_renderer_add_pass(soc_renderer* r, const soc_pass_desc* d, soc_pass_callback fn, void* user,
                                     const char* before) {
    if (!r || !d || !fn || !d->name || !d->name[0])
        return set_error(SOC_E_INVALID_ARG, "soc_renderer_add_pass: null renderer, descriptor, callback or name");
    return register_user_pass(r, d, [r, fn, user](const soc_globals* g, hipStream_t s) {
        const soc_frame_images v = callback_view(r);
        const int32_t rc = fn(user, g, &v, (soc_stream)s);
        return rc ? set_error(rc, "caller pass failed with %d", (int)rc) : (int)SOC_OK;
    }, before);
}

// ScreenSpaceReflectionTask as the reference registers it (renderer.cpp:1081-1092: after SSAOBlur, before
// CloudRendering), through the caller-pass machinery, so it is re-inserted by every graph rebuild.
extern "C" int soc_renderer_add_screen_space_reflection(soc_renderer* r, soc_img metallic_roughness, soc_img target,
                                                        soc_img steps, int32_t metallic_roughness_resource,
                                                        int32_t target_resource, uint32_t pass_flags, const char* before) {
    const char* fn = "soc_renderer_add_screen_space_reflection";
    if (!r) return set_error(SOC_E_INVALID_ARG, "%s: null renderer", fn);
    if (pass_flags & ~(uint32_t)SOC_PASS_ASYNC) return set_error(SOC_E_INVALID_ARG, "%s: pass_flags must be 0 or SOC_PASS_ASYNC", fn);
    for (int32_t id : {metallic_roughness_resource, target_resource})
        if (id < SOC_RES_USER0 || id >= SOC_RES_COUNT)
            return set_error(SOC_E_INVALID_ARG, "%s: bad resource id %d (SOC_RES_USER0 .. SOC_RES_USER0 + 31)", fn, id);
    if (metallic_roughness_resource == target_resource)
        return set_error(SOC_E_INVALID_ARG, "%s: the metallic-roughness image and the target need two resource ids", fn);
    int rc = check_img(metallic_roughness, SOC_FMT_RGBA16F, fn, "metallic_roughness");
    if (!rc) rc = check_img(target, SOC_FMT_RGBA16F, fn, "target");
    if (!rc && steps.data) rc = check_img(steps, SOC_FMT_R8_UNORM, fn, "steps");
    if (rc) return rc;
    const soc_img* same[] = {&metallic_roughness, &target, &steps};
    for (const soc_img* im : same)
        if (im->data && (im->width != r->img.depth.width || im->height != r->img.depth.height))
            return set_error(SOC_E_SHAPE, "%s: image is %dx%d, the frame's depth %dx%d", fn, im->width, im->height,
                             r->img.depth.width, r->img.depth.height);
    soc_pass_desc d{};
    d.name = "ScreenSpaceReflection";
    d.group = "Screen Space Reflections";
    d.phase = SOC_PHASE_PRE_EXPOSURE;
    d.flags = pass_flags;
    d.read_count = 4;
    d.reads[0] = SOC_RES_ALBEDO;
    d.reads[1] = SOC_RES_NORMAL;
    d.reads[2] = SOC_RES_DEPTH;
    d.reads[3] = metallic_roughness_resource;
    d.write_count = 1;
    d.writes[0] = target_resource;
    return register_user_pass(r, &d, [r, metallic_roughness, target, steps](const soc_globals* g, hipStream_t s) {
        return soc_screen_space_reflection(g, r->img.depth, r->img.normal, r->img.albedo, metallic_roughness, target, steps,
                                           (soc_stream)s);
    }, before ? before : "CloudRendering", before == nullptr);
}

// The reference's BlitImageToImage + MipMapping - i and DepthOfField (renderer.cpp:1119-1153: after Composition, before
// GenerateLuminanceHistogram) as two library-owned passes through the caller-pass machinery.
extern "C" int soc_renderer_add_depth_of_field(soc_renderer* r, soc_img chain, int32_t chain_resource, const char* before) {
    const char* fn = "soc_renderer_add_depth_of_field";
    if (!r) return set_error(SOC_E_INVALID_ARG, "%s: null renderer", fn);
    if (!(r->flags & SOC_RENDERER_UNFUSED_HISTOGRAM))
        return set_error(SOC_E_INVALID_ARG,
                         "%s: the renderer needs SOC_RENDERER_UNFUSED_HISTOGRAM: the fused Composition+GenerateLuminanceHistogram "
                         "pass bins the colour before the blur, the reference's histogram reads the blurred colour", fn);
    if (chain_resource < SOC_RES_USER0 || chain_resource >= SOC_RES_COUNT)
        return set_error(SOC_E_INVALID_ARG, "%s: bad resource id %d (SOC_RES_USER0 .. SOC_RES_USER0 + 31)", fn, chain_resource);
    const int rc = check_img(chain, SOC_FMT_RGBA16F, fn, "chain");
    if (rc) return rc;
    const soc_img& color = r->img.color;
    if (chain.width != color.width || chain.height != color.height)
        return set_error(SOC_E_SHAPE, "%s: chain is %dx%d, the frame's colour %dx%d", fn, chain.width, chain.height, color.width,
                         color.height);
    const size_t bytes = soc_depth_of_field_chain_bytes(chain.width, chain.height, chain.pitch_bytes);
    if (!bytes) return set_error(SOC_E_INVALID_ARG, "%s: extent %dx%d above 8192", fn, chain.width, chain.height);
    const char* c0 = static_cast<const char*>(color.data);
    const char* c1 = c0 + (size_t)color.pitch_bytes * (size_t)(color.height - 1) + (size_t)color.width * 8;
    const char* b0 = static_cast<const char*>(chain.data);
    if (c0 < b0 + bytes && b0 < c1)
        return set_error(SOC_E_INVALID_ARG, "%s: the frame's colour may not alias the chain's allocation", fn);
    const char* anchor = before ? before : "GenerateLuminanceHistogram";
    soc_pass_desc d{};
    d.name = "MipMapping";
    d.group = "Depth Of Field";
    d.phase = SOC_PHASE_PRE_EXPOSURE;
    d.read_count = 1;
    d.reads[0] = SOC_RES_COLOR;
    d.write_count = 1;
    d.writes[0] = chain_resource;
    int rc2 = register_user_pass(r, &d, [r, chain](const soc_globals*, hipStream_t s) {
        return soc_depth_of_field_mips(r->img.color, chain, (soc_stream)s);
    }, anchor);
    if (rc2) return rc2;
    d.name = "DepthOfField";
    d.read_count = 2;
    d.reads[0] = chain_resource;
    d.reads[1] = SOC_RES_DEPTH;
    d.writes[0] = SOC_RES_COLOR;
    rc2 = register_user_pass(r, &d, [r, chain](const soc_globals* g, hipStream_t s) {
        return soc_depth_of_field(g, r->img.depth, chain, r->img.color, (soc_stream)s);
    }, anchor);
    // roll the first pass back too (register_user_pass set the error; its own roll-back left "MipMapping" in)
    if (rc2) drop_last_user_pass(r);
    return rc2;
}

extern "C" int soc_renderer_pass_uses(const soc_renderer* r, int32_t i, uint64_t* reads, uint64_t* writes) {
    if (!r || i < 0 || i >= (int32_t)r->passes.size() || !reads || !writes)
        return set_error(SOC_E_INVALID_ARG, "soc_renderer_pass_uses: bad arguments");
    *reads = r->passes[i].reads;
    *writes = r->passes[i].writes;
    return SOC_OK;
}

// Pass i's in-frame (deps) or ring (carry) edges into `out`; the count, which may exceed `cap`.
static int32_t pass_edges(const char* fn, const soc_renderer* r, int32_t i, std::vector<int> soc_renderer::Pass::*edges,
                          int32_t* out, int32_t cap) {
    if (!r || i < 0 || i >= (int32_t)r->passes.size() || cap < 0 || (cap > 0 && !out))
        return set_error(SOC_E_INVALID_ARG, "%s: bad arguments", fn);
    const auto& d = r->passes[i].*edges;
    for (int k = 0; k < (int)d.size() && k < cap; ++k) out[k] = d[k];
    return (int32_t)d.size();
}

extern "C" int32_t soc_renderer_pass_dependencies(const soc_renderer* r, int32_t i, int32_t* out, int32_t cap) {
    return pass_edges("soc_renderer_pass_dependencies", r, i, &soc_renderer::Pass::deps, out, cap);
}

extern "C" int32_t soc_renderer_pass_carry_dependencies(const soc_renderer* r, int32_t i, int32_t* out, int32_t cap) {
    return pass_edges("soc_renderer_pass_carry_dependencies", r, i, &soc_renderer::Pass::carry, out, cap);
}

extern "C" int32_t soc_renderer_pass_lane(const soc_renderer* r, int32_t i) {
    if (!r || i < 0 || i >= (int32_t)r->passes.size()) return set_error(SOC_E_INVALID_ARG, "soc_renderer_pass_lane: bad index");
    return (r->passes[i].flags & SOC_PASS_ASYNC) ? 1 : 0;
}

extern "C" int32_t soc_renderer_pass_count(const soc_renderer* r) { return r ? (int32_t)r->passes.size() : 0; }

extern "C" const char* soc_renderer_pass_name(const soc_renderer* r, int32_t i) {
    if (!r || i < 0 || i >= (int32_t)r->passes.size()) return nullptr;
    return r->passes[i].name.c_str();
}

extern "C" const char* soc_renderer_pass_group(const soc_renderer* r, int32_t i) {
    if (!r || i < 0 || i >= (int32_t)r->passes.size()) return nullptr;
    return r->passes[i].group.c_str();
}

extern "C" int soc_renderer_set_alpha_mask(soc_renderer* r, int32_t enable) {
    if (!r) return set_error(SOC_E_INVALID_ARG, "soc_renderer_set_alpha_mask: null renderer");
    r->alpha_mask = enable != 0;   // read by DepthPrepass and SunShadowDraw when a frame runs: nothing is rebuilt
    return SOC_OK;
}
