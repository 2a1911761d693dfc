// clouds_plan.hpp — what the planner of a CloudRendering call (clouds_plan.cpp, host only, no HIP call) and its issuer
// (clouds.hip) share: the kernel-argument structs, the constants the host decisions use, the renderer-owned CloudState
// (cloud_state.hpp, which is all renderer.hpp needs), and the plan itself.
#pragma once

#include <algorithm>

#include "cloud_state.hpp"
#include "soc_internal.hpp"

namespace soc {

constexpr int kNoise = 64, kNoiseMask = 63;
// LDS quad table: 81 x 81 entries (64 + the 17-texel tap offset), so the second tap of get_3d_noise is
// the first tap's address plus a constant (an immediate ds_read offset) with no wrap arithmetic.
constexpr int kTap2 = 17, kTW = kNoise + kTap2, kTable = kTW * kTW;
// the quad tables padded to whole 16-B chunks (prebuilt in the workspace by clouds_od_lut, copied into LDS)
constexpr int kTableU32 = (kTable + 3) & ~3, kTableU2 = (kTable + 1) & ~1;
// the row table (RowF): one f16 pair per texel position of 82 rows (a quad's bottom row is the next row's entry)
constexpr int kRowTable = (kTW + 1) * kTW, kRowU32 = (kRowTable + 3) & ~3;
constexpr int kTableBuild = kRowU32 > kTableU32 ? kRowU32 : kTableU32;   // entries clouds_od_lut builds
constexpr float kRPlanet = 6371e3f;
constexpr int kOdR = 256, kOdM = 512;                                // the secondary-ray optical-depth table's grid
constexpr int kSvT = 128, kSvU = 64, kSvEntries = 3 * kSvT * kSvU;   // the sky-view table
constexpr int TX = 16, TY = 16;                                      // the single kernel's pixel tile
constexpr int kClassifyTiles = 4;
constexpr int kShards = 8;
// clouds_sunvis workgroup: 512 lanes (the 26 KiB noise table caps residency at 6 workgroups per CU: 512 lanes give the
// full 8 waves per SIMD); its launch bound
constexpr uint32_t kSunvisLanes = 512;
// density workgroups the od scratch is sized for: the resident set (6 per CU on 256 CUs is 1536) times the largest grid
// multiplier used (2: a sky-bound frame's density grid), 24 KiB each (4096 held 48 MiB more than any grid uses)
constexpr size_t kDensityBlocks = 3072;

struct CloudParams {
    Mat4 inv_proj, inv_view;
    float sun[3];      // -sun_info.direction
    float cam[3];
    float res_x_m1, res_y_m1;  // resolution - 1
    float r_res_x_m1, r_res_y_m1;  // recip_rn(resolution - 1) for the ray uv x / (W - 1) (div_rn)
    float elapsed;
    float sun_factor;  // max(min(|sun.x|, |sun.z|) + sun.y, 0)
    int res_x, res_y;
};

struct OdLut {
    const float2* t;   // [kOdR][kOdM] (log2 odR, log2 odM); nullptr: no table
    float C2;
};

struct SkyTab {
    const float4* t;   // [3][kSvT][kSvU] x 2: (totalRlh.xyz, totalMie.x), (totalMie.yz, -, -); nullptr: no table
    float upx, upy, upz, shx, shy, shz, btx, bty, btz;   // frame: up = r0 / |r0|, the sun's horizontal direction, up x sh
    float eh, dl;
};

struct PairBufs {
    uint32_t* counts;     // [kShards] pair counts (workspace counter block)
    uint32_t* pairs;      // [kShards * cap] (list index << 5) | step
    float* od;            // [kShards * cap] od of each pair's step (clouds_density)
    float* vis;           // [kShards * cap] sun visibility of each pair's step (clouds_sunvis); od and vis in two dense
                          // arrays (round 5: one float2 array took each kernel's 4-byte writes at an 8-byte stride, so
                          // every written line was half written)
    uint32_t* pix_mask;   // [W*H] per list entry: dense-step mask | kInline
    uint32_t* batch_base; // [W*H/256] per 256-entry batch: physical index of its first pair | kInline
    float4* geom;         // [W*H] x 2 per list entry: (start, dither), (inc, stepLength) of its march (density
                          // writes it for upward rays when store_geom; sunvis and resolve read it instead of re-deriving
                          // it; store_geom == 0: they re-derive it from the list entry, the same bits)
    float* od_tmp;        // [od_blocks][24][256]: per density workgroup, the od of its current batch's dense steps until
                          // their pair slots are known; density then stores od in od[slot], and sunvis only adds vis
    const uint32_t* noise_quads;  // [kTableU32] the frame's noise quad table (clouds_od_lut), or nullptr: stage_noise
    const uint2* noise_wide;      // [kTableU2] the same quads in float form (stage_noise_wide)
    const uint32_t* noise_rows;   // [kRowU32] the row table (stage_noise_rows)
    uint32_t store_geom;  // tuning knob SOC_CLOUDS_GEOM
    uint32_t od_blocks;   // density workgroups the od scratch holds (the density grid is clamped to it)
    uint32_t n;           // list capacity (W*H)
    uint32_t cap;         // pairs per shard
};

// Workspace: counters (256 B: [0] sky pixels, [8..15] pair counts per shard) | sky list (u32) |
// atmosphere (float4) | per-pixel dense mask (u32) | per-batch first pair (u32) | march geometry (2 float4) | pairs (u32) |
// od per pair (float) | vis per pair (float) | od scratch of the density workgroups (24 x 256 float each, at most kDensityBlocks) |
// the secondary-ray optical-depth table (kOdR x kOdM float2, 1 MiB) | sky-view table | noise tables |
// the second counter block (256 B).
// Pair capacity 2 per pixel of the image (8 shards).
// Per 256-entry batch of the list: the physical index of its first pair (or kInline).
struct CloudWs {
    uint32_t* counter;
    uint32_t* list;
    float4* atmos;
    PairBufs pb;
    float2* od_lut;   // secondary-ray optical-depth table (kOdR x kOdM)
    uint32_t* noise_quads;   // [kTableU32] noise quad tables (clouds_od_lut)
    uint2* noise_wide;       // [kTableU2]
    uint32_t* noise_rows;    // [kRowU32]
    float4* sky_tab;  // sky-view table (kSvEntries x 2 float4)
    uint32_t* counter_b;     // the second counter block (a renderer's frames alternate between the two)
    size_t bytes;
};
// Address arithmetic only: nothing is dereferenced (base may be null for the size).
inline CloudWs cloud_ws_layout(void* base, size_t n) {
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    char* b = static_cast<char*>(base);
    CloudWs w;
    size_t off = 256;
    w.counter = reinterpret_cast<uint32_t*>(b);
    w.list = reinterpret_cast<uint32_t*>(b + off);
    off = al(off + n * 4);
    w.atmos = reinterpret_cast<float4*>(b + off);
    off = al(off + n * 16);
    w.pb.counts = w.counter + 8;
    w.pb.pix_mask = reinterpret_cast<uint32_t*>(b + off);
    off = al(off + n * 4);
    w.pb.batch_base = reinterpret_cast<uint32_t*>(b + off);
    off = al(off + (n / 256 + 1) * 4);
    w.pb.geom = reinterpret_cast<float4*>(b + off);
    off = al(off + n * 32);
    w.pb.cap = (uint32_t)((2 * n + kShards - 1) / kShards);
    w.pb.pairs = reinterpret_cast<uint32_t*>(b + off);
    off = al(off + (size_t)kShards * w.pb.cap * 4);
    w.pb.od = reinterpret_cast<float*>(b + off);
    off = al(off + (size_t)kShards * w.pb.cap * 4);
    w.pb.vis = reinterpret_cast<float*>(b + off);
    off = al(off + (size_t)kShards * w.pb.cap * 4);
    w.pb.od_tmp = reinterpret_cast<float*>(b + off);
    w.pb.od_blocks = (uint32_t)std::min<size_t>(kDensityBlocks, (n + 255) / 256);
    w.pb.n = (uint32_t)n;
    off = al(off + (size_t)w.pb.od_blocks * 24 * 256 * 4);
    w.od_lut = reinterpret_cast<float2*>(b + off);
    off = al(off + (size_t)kOdR * kOdM * sizeof(float2));
    w.sky_tab = reinterpret_cast<float4*>(b + off);
    off = al(off + (size_t)kSvEntries * 2 * sizeof(float4));
    w.noise_quads = reinterpret_cast<uint32_t*>(b + off);
    off = al(off + (size_t)kTableU32 * 4);
    w.noise_wide = reinterpret_cast<uint2*>(b + off);
    off = al(off + (size_t)kTableU2 * 8);
    w.noise_rows = reinterpret_cast<uint32_t*>(b + off);
    off = al(off + (size_t)kRowU32 * 4);
    w.counter_b = reinterpret_cast<uint32_t*>(b + off);
    off += 256;
    w.bytes = off;
    return w;
}

// Workgroups resident on the device of the six kernels whose grids are sized by it (one full wave set each).
struct CloudResidency {
    int atmos, density, sunvis_wide, sunvis_quads, sunvis_rows, resolve;
};

// The instantiation of each march kernel: the column of the issuer's [r8][form] table (clouds.hip, march_kernels, and
// the hook's text in clouds_plan.cpp name every form by its enumerator).
enum DensityForm : int { kDensityRows, kDensityBatch4, kDensityBatch8, kDensityBatch1, kDensityForms };
enum SunvisForm : int { kSunvisRows, kSunvisQuads, kSunvisWidePf, kSunvisWide, kSunvisForms };
enum ResolveForm : int { kResolveFold4, kResolveFold8, kResolveFold1, kResolveAtmos, kResolveForms };

// One call's decisions, in issue order. The pointers are addresses inside the caller's workspace (never dereferenced
// by the planner).
struct CloudPlan {
    bool launch;          // false: nothing is issued (an empty extent)
    bool single;          // no workspace: clouds_kernel alone, grid (gx, gy) of TX x TY tiles
    bool r8;              // the noise format: the row of the [r8][form] tables
    int W, H;             // min of the target's and the globals' extents
    CloudParams p;
    int single_gx, single_gy;
    CloudWs ws;           // laid out for the target's extent; pb.counts, pb.store_geom and pb.noise_* are the call's
    bool prime_blocks;    // both counter blocks are cleared first (a renderer's first cached frame on this workspace)
    bool build_tables;    // clouds_od_lut runs: blocks [0, lut_blocks) build the od table (or only clear the counter
    bool build_od, build_noise;   // block), the blocks after them the noise tables
    int lut_blocks, lut_grid;
    float C2;             // dot(pSun, pSun)
    int counter_block;    // the block this call counts in (0, 1)
    int zero_block;       // the block its classification clears for the next frame (0, 1; -1: none)
    int vec_store;        // the target's base and pitch are multiples of 16
    bool hoist;
    int classify_gx, classify_gy;
    bool classify_only;   // SOC_CLOUDS_PROFILE >= 4
    OdLut lut;
    bool sky_table;       // clouds_sky_table runs (st.t is set)
    SkyTab st;            // the basis is filled in whenever it was computed, also when the table is then dropped
    bool fold;            // the resolve looks the atmosphere up itself: no atmosphere kernel
    int atmos_pos;        // the atmosphere kernel before the density march (0), before the sun visibility (1), after it (2)
    int atmos_grid;       // its form: the table's (st.t) or the march's
    DensityForm density;
    SunvisForm sunvis;
    ResolveForm resolve;
    int density_grid, sunvis_grid, resolve_grid;
};

// Plans soc_cloud_rendering(g, depth, noise, target, workspace): no HIP call, no image or workspace pointer dereferenced.
// `profile`: SOC_CLOUDS_PROFILE of the caller's build. `state` (may be null) is advanced as by a call that is then issued.
int plan_clouds(const soc_globals* g, const soc_img& depth, const soc_img& noise, const soc_img& target, void* workspace,
                bool sky_bound, int profile, const CloudResidency& res, CloudState* state, CloudPlan& out);

}  // namespace soc
