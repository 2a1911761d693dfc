// renderer.hpp — struct soc_renderer and what render_graph.cpp (building the graph) and render_execute.cpp (running a
// frame of it) share. Not part of the ABI.
#pragma once

#include <functional>
#include <string>
#include <vector>

#include "cloud_state.hpp"
#include "soc_internal.hpp"

namespace soc {
// One step of a frame's plan (plan_frame, render_execute.cpp), in issue order.
struct FrameStep {
    enum Kind : uint8_t {
        Fork,       // record the fork on the caller's stream
        ForkWait,   // the second lane waits for the fork
        Wait,       // `lane` waits for pass `src`'s `done`: an in-frame dependency across the lanes
        RingWait,   // the same for a source of an earlier call (a ring edge, or an edge into another phase's call)
        Run,        // run `pass` on `lane`
        Record,     // record `pass`'s `done` on `lane`
        Join,       // the caller's stream waits for the second lane
    };
    Kind kind;
    uint8_t lane;   // 0 = the caller's stream, 1 = the renderer's second lane
    int16_t pass;   // the pass run, recorded or about to run (-1: none)
    int16_t src;    // Wait / RingWait: the pass waited for (-1 otherwise)
};
// plan_frame's result and its working arrays, kept by the renderer so that a frame allocates nothing once they have grown.
struct FramePlan {
    std::vector<FrameStep> steps;
    bool lanes = false;   // the call runs passes on the second lane
    std::vector<int> lane, order, ao, rest, pos;
    std::vector<char> needs_fork;
    std::vector<std::vector<int>> deps, ext;
};
}  // namespace soc

// =================================================================================================
// Render graph (renderer.cpp:929-1235, live passes only; SSR / Hi-Z / DOF are dead or disabled; SSR and DOF can be added
// as opt-in passes, soc_renderer_add_screen_space_reflection / soc_renderer_add_depth_of_field)
//
// Every pass declares the frame resources it reads and writes (the Daxa task-uses block,
// e.g. composition.inl:10-21). The graph keeps the registration order, which is the reference's
// add_task order, and derives from the uses what Daxa derives its barriers from: each pass's
// dependencies on earlier passes (RAW, WAR, WAW). On one HIP stream stream order already satisfies
// them; they matter for SOC_PASS_ASYNC passes, which run on a second stream of the renderer
// (the async-compute queue the reference leaves unused): such a pass waits only for the passes it
// depends on, and a pass on the caller's stream waits for it only if it depends on it.
// =================================================================================================
struct soc_renderer {
    using PassFn = std::function<int(const soc_globals*, hipStream_t)>;
    struct Pass {
        std::string name, group;
        int phase = SOC_PHASE_PRE_EXPOSURE;
        uint64_t reads = 0, writes = 0;
        uint32_t flags = 0;
        PassFn run;
        std::function<bool()> skip;   // true: the pass has no work this call (no launch, no timing)
        std::vector<int> deps;        // derived: earlier passes this one must follow
        std::vector<int> carry;       // derived: passes of the PREVIOUS frame this one must follow (ring edges)
        bool signal = false;          // derived: a pass of the other lane depends on this one (records `done`)
        bool timed = false;
        std::vector<hipEvent_t> ev0, ev1;  // timing ring of SOC_RENDERER_TIMING_RING frames
        int next = 0, count = 0, last = -1;
        hipEvent_t done = nullptr;    // cross-lane completion event (created on first use)
        bool done_recorded = false;   // `done` holds this pass's latest run
    };
    // A pass inserted by every graph rebuild: a caller's (soc_renderer_add_pass) or a library-owned one
    // (soc_renderer_add_screen_space_reflection, soc_renderer_add_depth_of_field). `run` is built by the registering entry
    // point; `before_prefix`: the anchor is the first pass whose name begins with `before`.
    struct UserPass {
        soc_pass_desc desc;
        std::string name, group, before;
        bool before_prefix = false;
        PassFn run;
    };
    soc_frame_images img{};
    soc_raster_scene scene{};
    bool has_scene = false;
    // soc_renderer_set_draw_scene: the raster head from a draw scene instead of `scene` (has_scene is set with either).
    // The struct and the draw array are copies (draw_scene.draws points into `draws`); of `scene` only materials,
    // material_count, shadow and visibility are used then.
    soc_draw_scene draw_scene{};
    std::vector<soc_draw> draws;
    bool has_draws = false;
    // soc_renderer_set_draw_motion: the caller's history array (draw_scene.transform_count entries, device) the motion
    // resolve reads as last frame's transforms and GBufferGeneration rewrites every frame; null = motion off.
    // motion_valid: the array holds the transforms of the previous GBufferGeneration (false until the first one).
    soc_transform* motion_prev = nullptr;
    bool motion_valid = false;
    // soc_renderer_set_terrain: DrawTerrain / SunShadowDrawTerrain over the head's images (a copy; shadow_mesh resolved to
    // the mesh the shadow pass draws). Kept across a change of head, dropped with it.
    soc_terrain_layer terrain{};
    bool has_terrain = false;
    std::vector<Pass> passes;
    std::vector<UserPass> user_passes;
    uint32_t flags = 0;
    int hist = 0;               // history slot read as "previous" this frame
    uint64_t total_pixels = 0;  // 0 = this frame
    int wide = 0;
    // soc_renderer_set_light_bounds: Composition launches the bounded kernels on this device record (null: unbounded)
    const void* light_bounds = nullptr;
    uint32_t light_flags = 0;
    // soc_renderer_set_alpha_mask: DepthPrepass and SunShadowDraw call the *_masked raster twins with the head's
    // material table (read when a frame runs: no pass is rebuilt, and the flag survives a change of head)
    bool alpha_mask = false;
    // soc_renderer_set_sun_cascades: a copy of the record; img.shadow is then its atlas, the shadow passes draw every
    // cascade into its slab and Composition launches the cascaded call
    soc_sun_cascades cascades{};
    bool has_cascades = false;
    // slab k of the atlas as an image of its own (rows [k * S, (k + 1) * S))
    soc_img cascade_slab(int k) const {
        soc_img s = img.shadow;
        s.data = static_cast<char*>(s.data) + (size_t)k * (size_t)cascades.map_size * (size_t)s.pitch_bytes;
        s.height = cascades.map_size;
        return s;
    }
    // pinned staging ring for the device globals upload (lights)
    soc_globals* staging = nullptr;
    hipEvent_t staging_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    int staging_slot = 0;
    // second lane (SOC_PASS_ASYNC passes: CloudRendering is VALU-bound and reads only depth and noise, so
    // it overlaps the memory-bound bloom / SSAO passes)
    bool async = true;
    int side_device = -1;
    hipStream_t side = nullptr;
    hipEvent_t fork_ev = nullptr, join_ev = nullptr;
    // the second lane's hardware queue (ensure_side_lane): a stream of high or low priority, so the lane never shares
    // the caller's queue. Auto mode (the default) times frames with each and keeps the faster: lane_q = {high, low},
    // side_queue = 1 (high) / 2 (low) once chosen, -1 while the probe runs; 0 = normal priority (shared pool).
    hipStream_t lane_q[2] = {nullptr, nullptr};
    int side_queue = -1;
    int probe_frames = 0;
    hipEvent_t probe_ev[16] = {};
    hipEvent_t switch_ev = nullptr;
    // 8 partial luminance histograms of the fused composition + histogram pass (renderer-owned, 8 KiB)
    uint32_t* hist_scratch = nullptr;
    // a raster workspace of the sun shadow draw's own, so it can run on the second lane beside the depth prepass and
    // the G-buffer (they share scene.workspace's screen vertices and entry lists otherwise)
    void* shadow_ws = nullptr;
    size_t shadow_ws_bytes = 0;
    // this execute call runs both phases: the resolve folds the partial histograms itself (no fold launch)
    bool fold_in_resolve = false;
    // sky split configured (graph) / active this frame (the pair path applies at the globals' resolution)
    bool sky_split = false, sky_split_active = false;
    bool bloom_in_comp = false;          // SOC_RENDERER_BLOOM_IN_COMPOSITION applies to this graph
    bool bloom_in_comp_ok = false;       // ... and the fused pair path applies at this frame's globals resolution
    // SOC_BLOOM_SPARSE. bloom_sparse: the graph allows it (bloom_in_comp, and Composition is the only pass besides the
    // chain's last stage that declares the bloom-output resource). Per frame, set before the passes are issued so that
    // both callbacks see one decision: bloom_sparse_frame, the last stage leaves proven-zero strips unwritten;
    // bloom_cells_frame, Composition is handed mip3 and proves its cells (that frame, or beside the in-kernel bloom).
    bool bloom_sparse = false, bloom_sparse_frame = false, bloom_cells_frame = false;
    // the caller's stream is ordered after all second-lane work of the previous call (its join or an equivalent wait)
    bool main_after_side = true;
    // SOC_RENDERER_STATIC_INPUTS: a call of this graph has completed, so the frame inputs the caller wrote before its
    // first call are ordered before the second lane (that call's fork). Until then every second-lane pass waits for the
    // fork, as without the flag (the first call after create or a graph rebuild may follow the caller's input writes).
    bool inputs_ordered = false;
    // CloudRendering's record of the clouds workspace between frames: which static tables it holds (and their keys) and
    // the alternating counter blocks. Owned by the renderer (not a host-side cache keyed on the workspace pointer: a
    // freed and reused allocation must not read as built).
    soc::CloudState clouds_state;
    soc::FramePlan plan;   // the current call's plan (soc_renderer_execute)
    // the image the bloom chain writes and Composition reads, and its resource id
    const soc_img& bloom_image() const { return img.bloom_output.data ? img.bloom_output : img.emissive; }
    int bloom_resource() const { return img.bloom_output.data ? SOC_RES_BLOOM_OUTPUT : SOC_RES_EMISSIVE; }
};

namespace soc {
// render_graph.cpp
void destroy_pass_events(soc_renderer* r);
// render_execute.cpp
void destroy_side_lane(soc_renderer* r);
bool sky_lane_high(const soc_renderer* r);
bool bloom_in_comp_active(const soc_renderer* r);
}  // namespace soc
