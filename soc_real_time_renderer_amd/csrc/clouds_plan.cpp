// clouds_plan.cpp — the planner of a CloudRendering call: the argument checks, CloudParams, the static-table state machine,
// the counter block, the sky-view basis, the SOC_CLOUDS_* knobs (kept per reload), and from them the kernel forms and grids that
// clouds.hip's issue_clouds launches. Host only: no HIP call, no image or workspace pointer dereferenced
// (tests/test_cloud_plan.py runs it without a GPU through soc_debug_plan_clouds).
#include "clouds_plan.hpp"

#include <cmath>
#include <cstring>

namespace soc {
namespace {

// The sky-view table's basis for the camera and the sun, in double precision: up = r0 / |r0|, the sun's horizontal
// direction sh, bt = up x sh, and the horizon's elevation eh. False: the camera is at or below the surface (no table).
bool sky_view_basis(const CloudParams& p, SkyTab& st) {
    const double r0x = (double)(0.0f + p.cam[0]), r0y = (double)(6372e3f + p.cam[1]), r0z = (double)(0.0f + p.cam[2]);
    const double rl = std::sqrt(r0x * r0x + r0y * r0y + r0z * r0z);
    const double ux = r0x / rl, uy = r0y / rl, uz = r0z / rl;
    const double sx = p.sun[0], sy = p.sun[1], sz = p.sun[2], su = sx * ux + sy * uy + sz * uz;
    double hx = sx - su * ux, hy = sy - su * uy, hz = sz - su * uz, hl = std::sqrt(hx * hx + hy * hy + hz * hz);
    if (!(hl > 1e-9)) {   // sun at the zenith: any horizontal axis
        hx = uy; hy = -ux; hz = 0.0;
        hl = std::sqrt(hx * hx + hy * hy);
        if (!(hl > 1e-9)) { hx = 1.0; hy = 0.0; hz = 0.0; hl = 1.0; }
    }
    hx /= hl; hy /= hl; hz /= hl;
    const double bx = uy * hz - uz * hy, by = uz * hx - ux * hz, bz = ux * hy - uy * hx;
    const double q = (double)kRPlanet / rl;
    st.upx = (float)ux; st.upy = (float)uy; st.upz = (float)uz;
    st.shx = (float)hx; st.shy = (float)hy; st.shz = (float)hz;
    st.btx = (float)bx; st.bty = (float)by; st.btz = (float)bz;
    st.eh = q < 1.0 ? (float)std::sqrt(1.0 - q * q) : 0.0f;
    st.dl = 3e-5f;   // margin inside each branch: the fp32 discriminant is ambiguous within ~1e-5 of the grazing elevation
    return st.eh > 4.0f * st.dl;
}

// The SOC_CLOUDS_* knobs with their defaults (each is described where plan_clouds uses it), read through tuning_knob once
// per thread and soc_tuning_reload() instead of fifteen locked lookups by name in every call: those took 2-3 us ahead of a
// frame's first clouds launch, which a 150 us frame showed (profiles/clouds_plan_bench_ab.txt).
struct CloudKnobs {
    int geom, od_lut, noise_table, static_tables, classify_hoist, grid_mult, atmos_pos,
        sky_table, atmos_fold, density_batch, density_rows, density_mult, sunvis_wide, sunvis_pf, resolve_batch;
};
const CloudKnobs& cloud_knobs() {
    thread_local uint32_t generation = 0;   // tuning_generation() is never 0
    thread_local CloudKnobs k;
    const uint32_t now = tuning_generation();
    if (generation != now) {
        k = CloudKnobs{tuning_knob("SOC_CLOUDS_GEOM", 1),
                       tuning_knob("SOC_CLOUDS_OD_LUT", 1),
                       tuning_knob("SOC_CLOUDS_NOISE_TABLE", 1),
                       tuning_knob("SOC_CLOUDS_STATIC_TABLES", -1),
                       tuning_knob("SOC_CLOUDS_CLASSIFY_HOIST", 0),
                       tuning_knob("SOC_CLOUDS_GRID_MULT", 2),
                       tuning_knob("SOC_CLOUDS_ATMOS_POS", -1),
                       tuning_knob("SOC_CLOUDS_SKY_TABLE", 1),
                       tuning_knob("SOC_CLOUDS_ATMOS_FOLD", 1),
                       tuning_knob("SOC_CLOUDS_DENSITY_BATCH", 8),
                       tuning_knob("SOC_CLOUDS_DENSITY_ROWS", 1),
                       tuning_knob("SOC_CLOUDS_DENSITY_MULT", 1),
                       tuning_knob("SOC_CLOUDS_SUNVIS_WIDE", 2),
                       tuning_knob("SOC_CLOUDS_SUNVIS_PF", 1),
                       tuning_knob("SOC_CLOUDS_RESOLVE_BATCH", 4)};
        generation = now;
    }
    return k;
}

// The static tables and the alternating counter blocks of a renderer's frame (`cached`), or what the per-call form
// leaves of them.
// Stateless (no `state`, soc_cloud_rendering; or SOC_CLOUDS_STATIC_TABLES=0): the tables are built on every call, by the
// kernel that also clears the call's counter block (block 0).
// A renderer's frames (`state`): both are static in real use (the od table depends only on C2 = dot(pSun, pSun), which
// changes when the sun is edited; the noise is an asset loaded once), so each is built when first needed and again
// only when its key changes (the bit pattern of C2; the noise image's data, format, pitch;
// soc_renderer_invalidate_cloud_tables for texels rewritten in place). The counter block then has no launch to clear
// it: frame N counts in block N & 1, and one workgroup of its clouds_classify clears block (N + 1) & 1, which frame
// N - 1 used last (all its kernels precede this frame's in stream order); both blocks are cleared when the renderer
// first uses the workspace this way. The classification runs over the whole image in every frame, so a frame
// without sky clears the next block too, and a sky frame after it starts from zero. (Not clouds_density: one more
// kernel argument took its scratch from 12 to 32 B per lane, +4.5 us at C3 and C4.)
void plan_tables(CloudState* state, bool cached, const soc_img& noise, void* workspace, bool use_lut, bool noise_tab,
                 CloudPlan& out) {
    out.build_od = use_lut;
    out.build_noise = noise_tab;
    out.counter_block = 0;
    out.zero_block = -1;
    if (cached) {
        if (state->workspace != workspace) {   // another workspace: nothing of the record holds
            state->invalidate_tables();
            state->blocks_primed = false;
            state->workspace = workspace;
        }
        out.prime_blocks = !state->blocks_primed;
        state->blocks_primed = true;
        uint32_t c2_bits;
        memcpy(&c2_bits, &out.C2, sizeof c2_bits);
        if (state->od_valid && state->c2_bits != c2_bits) state->od_valid = false;
        if (state->noise_valid && (state->noise_data != noise.data || state->noise_format != noise.format ||
                                   state->noise_pitch != noise.pitch_bytes))
            state->noise_valid = false;
        out.build_od = use_lut && !state->od_valid;
        out.build_noise = noise_tab && !state->noise_valid;
        if (out.build_od) {
            state->od_valid = true;
            state->c2_bits = c2_bits;
        }
        if (out.build_noise) {
            state->noise_valid = true;
            state->noise_data = noise.data;
            state->noise_format = noise.format;
            state->noise_pitch = noise.pitch_bytes;
        }
        out.counter_block = (int)(state->frame & 1u);
        out.zero_block = 1 - out.counter_block;
        state->frame++;
    } else if (state) {   // the per-call form leaves the blocks and the tables as any caller of the workspace would
        state->invalidate_tables();
        state->blocks_primed = false;
        state->workspace = nullptr;
    }
    // blocks [0, lut_blocks) build the od table (without it: one block, which only clears the counter block), the
    // blocks after them the noise tables. The cached form's block is already clear; the kernel clears it again.
    out.build_tables = !cached || out.build_od || out.build_noise;
    out.lut_blocks = out.build_od ? ceil_div(kOdR * kOdM, kWorkgroup) : 1;
    out.lut_grid = out.lut_blocks + (out.build_noise ? ceil_div(kTableBuild, kWorkgroup) : 0);
}

}  // namespace

int plan_clouds(const soc_globals* g, const soc_img& depth, const soc_img& noise, const soc_img& target, void* workspace,
                bool sky_bound, int profile, const CloudResidency& res, CloudState* state, CloudPlan& out) {
    static const char* P = "soc_cloud_rendering";
    out = CloudPlan{};
    if (!g) return set_error(SOC_E_INVALID_ARG, "%s: null globals", P);
    int rc = check_img(depth, SOC_FMT_D32F, P, "depth");
    if (!rc) rc = check_img(target, SOC_FMT_RGBA8_UNORM, P, "target");
    if (!rc) rc = check_img(noise, 0, P, "noise");
    if (rc) return rc;
    if (noise.format != SOC_FMT_R8_UNORM && noise.format != SOC_FMT_RGBA8_UNORM)
        return set_error(SOC_E_UNSUPPORTED, "%s: noise must be R8_UNORM or RGBA8_UNORM", P);
    if (noise.width != 64 || noise.height != 64)
        return set_error(SOC_E_SHAPE, "%s: noise texture must be 64x64 (assets/Clouds/noise.png)", P);
    CloudParams& p = out.p;
    p.inv_proj = mat4(g->camera_inverse_projection_matrix);
    p.inv_view = mat4(g->camera_inverse_view_matrix);
    for (int i = 0; i < 3; ++i) {
        p.sun[i] = -g->sun_info.direction[i];
        p.cam[i] = g->camera_position[i];
    }
    p.res_x = g->resolution[0];
    p.res_y = g->resolution[1];
    p.res_x_m1 = (float)g->resolution[0] - 1.0f;
    p.res_y_m1 = (float)g->resolution[1] - 1.0f;
    p.r_res_x_m1 = recip_rn(g->resolution[0] - 1);
    p.r_res_y_m1 = recip_rn(g->resolution[1] - 1);
    p.elapsed = g->elapsed_time;
    p.sun_factor = fmaxf(fminf(fabsf(p.sun[0]), fabsf(p.sun[2])) + p.sun[1], 0.0f);
    const int W = out.W = std::min(target.width, p.res_x), H = out.H = std::min(target.height, p.res_y);
    if (W <= 0 || H <= 0) return SOC_OK;
    if (W > 65535 || H > 65535) return set_error(SOC_E_SHAPE, "%s: extent above 65535", P);
    out.launch = true;
    out.r8 = noise.format == SOC_FMT_R8_UNORM;
    if (!workspace) {
        out.single = true;
        out.single_gx = ceil_div(W, TX);
        out.single_gy = ceil_div(H, TY);
        return SOC_OK;
    }
    const CloudKnobs& knob = cloud_knobs();
    // the caller sized the workspace for the target extent (soc_cloud_rendering_workspace_size)
    CloudWs& ws = out.ws = cloud_ws_layout(workspace, (size_t)target.width * (size_t)target.height);
    ws.pb.store_geom = (uint32_t)knob.geom;
    // the secondary-ray table (SOC_CLOUDS_OD_LUT=0: march every secondary ray, the single-lane kernel's bits) and the
    // noise quad tables (SOC_CLOUDS_NOISE_TABLE=0: each march workgroup stages them from the noise image texel by texel,
    // the same bytes), both built by clouds_od_lut.
    const bool use_lut = profile < 4 && knob.od_lut;
    const bool noise_tab = knob.noise_table != 0;
    out.C2 = p.sun[0] * p.sun[0] + p.sun[1] * p.sun[1] + p.sun[2] * p.sun[2];   // dot3(pSun, pSun)
    out.lut = use_lut ? OdLut{ws.od_lut, out.C2} : OdLut{nullptr, 0.0f};
    ws.pb.noise_quads = noise_tab ? ws.noise_quads : nullptr;
    ws.pb.noise_wide = noise_tab ? ws.noise_wide : nullptr;
    ws.pb.noise_rows = noise_tab ? ws.noise_rows : nullptr;
    // SOC_CLOUDS_STATIC_TABLES: 1 the static form, 0 the per-call build, default (-1) the static form except in a
    // sky-bound frame above 1440p (the render graph's high-priority sky lane, as the atmosphere's position below): the
    // C4 frame at 3840x2160 is 0.5 % slower without the 13 us build launch ahead of the classification (1498-1504 fps
    // against 1506-1511 with it, five alternating runs: the lane's kernels start earlier, and clouds_sunvis then runs
    // 12 us longer beside the main lane), while the sky-bound C2 frame at 1920x1080 gains 3 % and C3 1.5 %
    // (profiles/r07_ab_static_tables.txt). The same bits in every form.
    const bool above_1440p = (long long)W * H > 2560LL * 1440LL;
    const int static_knob = knob.static_tables;
    const bool static_tables = static_knob >= 0 ? static_knob != 0 : !(sky_bound && above_1440p);
    plan_tables(state, state && profile < 4 && static_tables, noise, workspace, use_lut, noise_tab, out);
    ws.pb.counts = (out.counter_block ? ws.counter_b : ws.counter) + 8;
    out.vec_store = (target.pitch_bytes % 16 == 0) && (reinterpret_cast<uintptr_t>(target.data) % 16 == 0);
    out.hoist = sky_bound || knob.classify_hoist;
    out.classify_gx = ceil_div(W, 64);
    out.classify_gy = ceil_div(H, 16 * kClassifyTiles);
    out.classify_only = profile >= 4;
    if (out.classify_only) return SOC_OK;
    // One resident wave set per kernel, grid-stride over the list / pairs: the long per-item work is
    // balanced over all SIMDs instead of running as a second, partially filled round.
    // SOC_CLOUDS_GRID_MULT: the sun-visibility and resolve grids as this many times the resident wave set (1: one
    // persistent set; more: workgroups queue behind each other, so the dispatcher can place the main lane's workgroups
    // between them instead of on what a persistent set leaves). The same bits at any grid. Default 2: C3 1678 -> 1699 fps,
    // C2 5313 -> 5526, C4 unchanged; 3 measured C3 1644, C4 1342; 4 / 8: C3 1646 / 1629 (profiles/r05_ab_clouds_grid_mult.txt).
    const long long blocks = ((long long)W * H + 255) / 256;
    const int gmul = std::max(1, knob.grid_mult);
    auto grid = [&](int resident, int mul) {
        return (int)std::max(1LL, std::min<long long>((long long)resident * mul, blocks));
    };
    // Position of the atmosphere kernel in the lane (it feeds only the resolve): before the density march (0), before
    // the sun visibility (1) or after it (2). Default: after it above 1440p (C3 +0.7 %, C4 +5 % at 3840x2160: the
    // atmosphere's long transcendental run then overlaps the frame's TAA instead of its SSAO), first otherwise (C2
    // 1920x1080 -5 % after it); the same bits in every position (profiles/r03_ab_atmos_pos.txt, GPU identity test).
    const int apos_knob = knob.atmos_pos;
    out.atmos_pos = apos_knob >= 0 ? apos_knob : (above_1440p ? 2 : 0);
    out.atmos_grid = grid(res.atmos, 1);
    // the frame's sky-view table (needs the secondary-ray table; SOC_CLOUDS_SKY_TABLE=0: every pixel evaluated)
    if (out.lut.t && knob.sky_table && sky_view_basis(p, out.st)) out.st.t = ws.sky_tab;
    out.sky_table = out.st.t != nullptr;
    // with the table the resolve looks the atmosphere up itself (SOC_CLOUDS_ATMOS_FOLD=0: the atmosphere kernel from the table)
    out.fold = out.sky_table && knob.atmos_fold;
    // SOC_CLOUDS_DENSITY_ROWS (default 1): the density kernel's noise from the float-form row table (RowF; the same bits);
    // otherwise SOC_CLOUDS_DENSITY_BATCH: its od scratch read back in batches of this many steps (1: one dense step at a time)
    const int db = knob.density_batch;
    out.density = knob.density_rows != 0 ? kDensityRows
                  : db == 4 ? kDensityBatch4 : db == 8 ? kDensityBatch8 : kDensityBatch1;
    // one od scratch per workgroup; SOC_CLOUDS_DENSITY_MULT: the grid as this many times the resident set (as gmul).
    // Default 1: 2 measured C3 1710 -> 1697 fps, C4 1321 -> 1358 (profiles/r05_ab_clouds_density_mult.txt)
    const int dmul = sky_bound ? 2 : std::max(1, knob.density_mult);
    out.density_grid = std::min(grid(res.density, dmul), (int)ws.pb.od_blocks);
    // the sun-visibility kernel's noise table (SOC_CLOUDS_SUNVIS_WIDE): 2 (default) the float-form row table (RowF, 26 KiB
    // per 512-lane workgroup: 8 waves per SIMD, and room on the CU for the main lane's SSAO tile; C3 1728 -> 1799 fps),
    // 1 the float-form quads (52 KiB, 6 waves per SIMD), 0 the byte quads (integer form, 26 KiB). The same bits.
    // SOC_CLOUDS_SUNVIS_PF (the float-form quads only): the next pair word loaded one iteration ahead
    const int sv_table = knob.sunvis_wide;
    out.sunvis = sv_table == 2 ? kSunvisRows
                 : sv_table == 0 ? kSunvisQuads
                 : knob.sunvis_pf != 0 ? kSunvisWidePf : kSunvisWide;
    out.sunvis_grid = grid(out.sunvis == kSunvisRows ? res.sunvis_rows
                           : out.sunvis == kSunvisQuads ? res.sunvis_quads : res.sunvis_wide, gmul);
    // the resolve's od / vis loads issued in batches of SOC_CLOUDS_RESOLVE_BATCH steps (1: one step at a time; the
    // folded form only)
    const int rb = knob.resolve_batch;
    out.resolve = !out.fold ? kResolveAtmos : rb == 4 ? kResolveFold4 : rb == 8 ? kResolveFold8 : kResolveFold1;
    out.resolve_grid = grid(res.resolve, gmul);
    return SOC_OK;
}

}  // namespace soc

using namespace soc;

// Test hooks (not in the public header). soc_debug_plan_clouds: the plan of soc_cloud_rendering(g, depth, noise, target,
// workspace) as text, without a HIP call: a header line (W, H, the list capacity the workspace is laid out for, the counter block, the block to zero, vec_store,
// store_geom, the noise-table switches, the od table, and the bit patterns of C2 and of the sky-view basis), then one line
// per step issue_clouds would take, in issue order: "memset<TAB>block<TAB>bytes" or "kernel<TAB>name<TAB>form<TAB>grid
// <TAB>block"; with a `state` (soc_debug_cloud_state_bytes() zero bytes are a fresh one; null: the stateless entry) a last
// line with the record as the call leaves it (after a refused call that line alone). `residency`: the six resident-set
// sizes in CloudResidency's order. Returns the text's length (truncated to cap - 1 characters in `buf`), or an error code.
extern "C" size_t soc_debug_cloud_state_bytes(void) { return sizeof(CloudState); }

extern "C" int64_t soc_debug_plan_clouds(const soc_globals* g, soc_img depth, soc_img noise, soc_img target, void* workspace,
                                         int32_t sky_bound, const int32_t residency[6], void* state_bytes, char* buf,
                                         size_t cap) {
    if (!residency) return set_error(SOC_E_INVALID_ARG, "soc_debug_plan_clouds: null residency");
    const CloudResidency res{residency[0], residency[1], residency[2], residency[3], residency[4], residency[5]};
    CloudState* state = static_cast<CloudState*>(state_bytes);
    CloudPlan pl;
    const int rc = plan_clouds(g, depth, noise, target, workspace, sky_bound != 0, 0, res, state, pl);
    if (rc && state) {   // as cloud_rendering_launch
        state->blocks_primed = false;
        state->invalidate_tables();
    }
    std::string out;
    char line[512];
    auto bits = [](float v) {
        uint32_t u;
        memcpy(&u, &v, sizeof u);
        return u;
    };
    auto kernel = [&](const char* name, const std::string& form, int gx, int gy, int bx, int by) {
        std::snprintf(line, sizeof line, "kernel\t%s\t%s\t%dx%dx1\t%dx%dx1\n", name, form.c_str(), gx, gy, bx, by);
        out += line;
    };
    const std::string fmt = pl.r8 ? "r8" : "rgba8";
    if (!rc && pl.launch && pl.single) {
        std::snprintf(line, sizeof line, "clouds\t%d\t%d\tsingle\n", pl.W, pl.H);
        out += line;
        kernel("clouds_kernel", fmt, pl.single_gx, pl.single_gy, TX, TY);
    } else if (!rc && pl.launch) {
        // each form by name, as the issuer's table (clouds.hip, march_kernels) names them
        auto density = [](DensityForm f) {
            return f == kDensityRows ? " batch8 rows" : f == kDensityBatch4 ? " batch4" : f == kDensityBatch8 ? " batch8" : " batch1";
        };
        auto sunvis = [](SunvisForm f) {
            return f == kSunvisRows ? " rows pf" : f == kSunvisQuads ? " quads pf" : f == kSunvisWidePf ? " wide pf" : " wide";
        };
        auto resolve = [](ResolveForm f) {
            return f == kResolveFold4 ? " fold batch4" : f == kResolveFold8 ? " fold batch8"
                   : f == kResolveFold1 ? " fold batch1" : " atmos batch1";
        };
        const SkyTab& st = pl.st;
        std::snprintf(line, sizeof line,
                      "clouds\t%d\t%d\tlist=%u\tcounter=%d\tzero=%d\tvec_store=%d\tstore_geom=%u\tnoise_tables=%d%d%d\tod_table=%d\t"
                      "C2=%08x\tsky=%d:%08x,%08x,%08x,%08x,%08x,%08x,%08x,%08x,%08x,%08x,%08x\n",
                      pl.W, pl.H, pl.ws.pb.n, pl.counter_block, pl.zero_block, pl.vec_store, pl.ws.pb.store_geom,
                      pl.ws.pb.noise_quads != nullptr, pl.ws.pb.noise_wide != nullptr, pl.ws.pb.noise_rows != nullptr,
                      pl.lut.t != nullptr, bits(pl.C2), st.t != nullptr, bits(st.upx), bits(st.upy), bits(st.upz),
                      bits(st.shx), bits(st.shy), bits(st.shz), bits(st.btx), bits(st.bty), bits(st.btz), bits(st.eh),
                      bits(st.dl));
        out += line;
        if (pl.prime_blocks) out += "memset\tcounter0\t256\nmemset\tcounter1\t256\n";
        if (pl.build_tables)
            kernel("clouds_od_lut", fmt + " od=" + std::to_string(pl.build_od) + " noise=" + std::to_string(pl.build_noise) +
                                        " lut_blocks=" + std::to_string(pl.lut_blocks), pl.lut_grid, 1, kWorkgroup, 1);
        kernel("clouds_classify", pl.hoist ? "hoist" : "plain", pl.classify_gx, pl.classify_gy, kWorkgroup, 1);
        if (!pl.classify_only) {
            auto atmos = [&](int pos) {
                if (pl.atmos_pos == pos && !pl.fold)
                    kernel("clouds_atmosphere", pl.sky_table ? "table" : "march", pl.atmos_grid, 1, kWorkgroup, 1);
            };
            if (pl.sky_table) kernel("clouds_sky_table", "-", ceil_div(kSvEntries, kWorkgroup), 1, kWorkgroup, 1);
            atmos(0);
            kernel("clouds_density", fmt + density(pl.density), pl.density_grid, 1, kWorkgroup, 1);
            atmos(1);
            kernel("clouds_sunvis", fmt + sunvis(pl.sunvis), pl.sunvis_grid, 1, kSunvisLanes, 1);
            atmos(2);
            kernel("clouds_resolve", fmt + resolve(pl.resolve), pl.resolve_grid, 1, kWorkgroup, 1);
        }
    }
    if (state) {
        std::snprintf(line, sizeof line, "state\tod=%d\tnoise=%d\tc2=%08x\tnoise_data=%llx\tformat=%d\tpitch=%d\tworkspace=%llx\t"
                      "primed=%d\tframe=%u\n", state->od_valid, state->noise_valid, state->c2_bits,
                      (unsigned long long)reinterpret_cast<uintptr_t>(state->noise_data), state->noise_format,
                      state->noise_pitch, (unsigned long long)reinterpret_cast<uintptr_t>(state->workspace),
                      state->blocks_primed, state->frame);
        out += line;
    }
    const int64_t n = copy_text(out, buf, cap);
    return rc ? rc : n;
}
