// post_plan.hpp — what the planners of the TAA, SSAO and bloom calls (post_plan.cpp, host only, no HIP call) and their
// issuers (taa.hip, ssao.hip, bloom_w.hip, bloom.hip) share: the kernel-argument structs, each kernel form as data and the
// plans.
#pragma once

#include "agx.hpp"
#include "soc_internal.hpp"

namespace soc {

// ---- TAA ---------------------------------------------------------------------------------------------------------------
struct TaaParams {
    float rw, rh;       // recip_rn(target extent) for the pixel-centre uv (div_rn)
    float pox, poy;     // 1 / resolution
    float accum0;       // min(0.1, frame_counter)
    int swz;            // XCD-aware tile order (pair path)
};
// Fused ToneMappingTask (tone_mapping.inl:145-176) epilogue: the resolved RGBA16F pair, exactly as it
// is stored, goes through the same AgX device function as tonemap_pair into an RGBA8_UNORM image.
struct TmOut {
    DImg out;
    const soc_auto_exposure* ae;
    TmParams p;
    int srgb;   // RGBA8_SRGB framebuffer: sRGB-encode on store
};

constexpr int kTaaBX = 64, kTaaBY = 4;   // taa_fast / taa_generic: one lane per pixel
constexpr int kTaaPairs = 64;            // output pairs per workgroup row (taa_lds)
constexpr int kTaaLdsRows = 4;           // rows per workgroup: 4 measured against 2 and 8 (profiles/r03_ab_taa_lds.txt)

// One TAA call as its entry point received it; tone_map: soc_temporal_antialiasing_tone_mapping (ae, output).
struct TaaCall {
    const soc_globals* g;
    soc_img target, current_color, previous_color, current_velocity, previous_velocity, depth, velocity_history_out;
    bool tone_map;
    const soc_auto_exposure* ae;
    soc_img output;
};
// taa_lds<TM, kTaaLdsRows, SF> (SF: kTaaLdsSf), taa_pair2<TM, NBR>, taa_fast, taa_generic
enum TaaKernel : int { kTaaLdsSf, kTaaLds, kTaaPair2N0, kTaaPair2N1, kTaaPair2N2, kTaaFast, kTaaGeneric, kTaaKernels };
struct TaaPlan {
    TaaKernel kernel;
    bool tm;             // the tone map is the kernel's epilogue (tmo)
    int grid_x, grid_y, block_x, block_y;
    DImg img[7];         // target, colour, history, velocity, velocity history, depth, velocity_history_out (null: none)
    TaaParams p;
    TmOut tmo;           // zeros unless tm
    bool tone_mapping_pass;   // not fused: soc_tone_mapping(g, target, ae, output) follows
};
// The checks in the entry points' order (SOC_OK, or the code with the message set), the kernel, the grid, the blocks.
int plan_taa(const TaaCall& c, TaaPlan& out);
// Plans the call and issues the plan on `stream` (taa.hip): what both entry points run.
int temporal_antialiasing(const TaaCall& c, soc_stream stream);

// ---- SSAO --------------------------------------------------------------------------------------------------------------
struct SsaoParams {
    Mat4 inv_proj;
    Mat4 proj;
    Mat4 view;
    float radius, bias, kernel_size_f;
    int ksize;     // loop bound, min(kernel_size, 26)
    int noise_w;   // textureSize(u_normal_image).x
    int swz;       // XCD-aware tile order (tuning knob SOC_SWZ_SSAO, see xcd_order; 0 = row-major)
    float rw, rh;  // recip_rn(target extent) for the pixel-centre uv (div_rn)
    // host-folded constants of the tap loop (plan_ssao_generation): the projection rows x, y, w scaled to texel space
    // (x 256 sub-texel steps on the sparse path), the texel-space centre and clamp bounds, 1 / kernel_size
    float pa[3][4];
    float c0x, c0y, tmx, tmy;
    float inv_ksize;
    float inv_radius;   // 1 / radius (the sparse path requires radius > 0)
};

#ifndef SOC_SSAO_TILE_TX
#define SOC_SSAO_TILE_TX 64   // A/B builds: the tile's half-res extent (a variant's ssao.hip passes its own to the planner)
#endif
#ifndef SOC_SSAO_TILE_TY
#define SOC_SSAO_TILE_TY 16
#endif
constexpr int kSsaoTX = SOC_SSAO_TILE_TX, kSsaoTY = SOC_SSAO_TILE_TY, kSsaoTileLanes = kSsaoTX * kSsaoTY;

// ssao_pipe_kernel<PERSP>, ssao_lds_kernel<EARLY>, the gather ssao_kernel<TABLE, SPARSE_IP, FULL>
enum SsaoKernel : int { kSsaoPipe, kSsaoLds, kSsaoGather };
struct SsaoPlan {
    SsaoKernel kernel;
    bool persp;              // kSsaoPipe
    int early;               // kSsaoLds: 0, 1, 2
    bool table, sip, full;   // kSsaoGather
    int grid_x, grid_y, block_x;   // the tile grid of tx * ty lanes, or 32 x 8 pixels per 256 lanes
    DImg depth, normal, target;
    const float2* noise;
    SsaoParams p;            // swz: 1 on the tiles, SOC_SWZ_SSAO on the gather kernel
};
// tx, ty: the tile of the issuing ssao.hip
int plan_ssao_generation(const soc_globals* g, const soc_img& depth, const soc_img& normal, const soc_img& target,
                         const float* noise_table, SsaoPlan& out, int tx = kSsaoTX, int ty = kSsaoTY);
struct SsaoBlurPlan {
    bool generic;            // extents differ (or exceed 8192): bilinear taps with steps tx, ty
    int grid_x, grid_y;      // blocks of 64 x 4
    DImg src, dst;
    float tx, ty;
};
int plan_ssao_blur(const soc_img& ssao, const soc_img& target, SsaoBlurPlan& out);
int check_ssao_prepare_noise(const soc_img& normal, const soc_img& target, const float* noise_table);

// ---- weighted bloom ----------------------------------------------------------------------------------------------------
// The chain's fixed-ratio fast paths apply when the four mips halve exactly (the reference's mip chain at even
// extents, renderer.cpp:492-513) and the extents fit the 8-bit fixed-point tap range.
bool bloom_fused_applicable(const soc_img& emissive, const soc_img* mips, int mip_count, const soc_img& output);
// The last stage may leave proven-zero strips unwritten (sparse_output): the register-form W4 with the zero skip, unless
// SOC_BLOOM_SPARSE=0 (the dense launches, for A/B).
bool bloom_sparse_applicable();

#ifndef SOC_BLOOM_UP10_ROWS
#define SOC_BLOOM_UP10_ROWS 16   // A/B builds: rows per wave of bloomw_up10r (a variant's bloom_w.hip passes its own)
#endif
constexpr int W2_OW = 16, W2_OH = 8;     // bloomw_down23: mip3 outputs per workgroup
constexpr int U_OW = 64, U_OH = 16;      // the tiled upsamples' outputs per workgroup
constexpr int R_OW = 62, R_TH = SOC_BLOOM_UP10_ROWS;   // bloomw_up10r: output columns and rows per wave
constexpr int w1_ow(int mode) { return mode ? 30 : 32; }        // bloomw_down01p<MODE>: mip1 outputs per workgroup
constexpr int w1_oh(int mode) { return mode == 2 ? 16 : 8; }

// bloomw_down01p<MODE, ZS>, bloomw_down23<REG>, bloomw_up32s<RUNS>, bloomw_up32, bloomw_up10r<ZS, SPARSE>, bloomw_up10s,
// bloomw_up10
enum BloomwKernel : int { kBwDown01p, kBwDown23, kBwUp32s, kBwUp32, kBwUp10r, kBwUp10s, kBwUp10 };
struct BloomwStage {
    BloomwKernel kernel;
    int f0, f1;              // the template arguments in the order above (0 where there is none)
    int grid_x, grid_y;      // blocks of kWorkgroup lanes
    DImg src, dst, m3;       // m3: bloomw_up10r's zero cells
    int a[4];                // the scalar arguments in the kernel's order: (ntx, nty), (w2, h2, swz), (w2, h2, vec, swz),
                             // (nwx, nwaves), (vec, swz, zero_skip), (vec, swz)
};
struct BloomwPlan {
    int n;
    BloomwStage st[4];
};
// stage: 0 the chain, 1..4 one stage. resident[mode * 2 + zs]: the workgroups of bloomw_down01p<mode, zs> resident on
// the device at once (the issuer's occupancy query). sparse_output: output strips proven zero from mips[3] are not
// written; refused, before anything is issued, unless bloom_sparse_applicable(). rows: the issuing bloom_w.hip's R_TH.
int plan_bloom_weighted(const soc_img& emissive, const soc_img* mips, const soc_img& output, int stage, bool sparse_output,
                        const int resident[6], BloomwPlan& out, int rows = R_TH);
// soc_bloom_weighted_stage's checks
int check_bloom_weighted_stage(const soc_img& emissive, const soc_img* mips, int mip_count, const soc_img& output, int stage);
// Plans and issues (bloom_w.hip); the images were checked by the caller (bloom_fused_applicable holds).
int bloom_weighted(const soc_img& emissive, const soc_img* mips, const soc_img& output, hipStream_t s, int stage,
                   bool sparse_output = false);

// ---- per-pass bloom ----------------------------------------------------------------------------------------------------
constexpr int kBloomBX = 64, kBloomBY = 4;
enum BloomKernel : int {
    kBloomDownSameQ, kBloomDownHalfW, kBloomDownGeneric, kBloomUpSameQ, kBloomUpDouble, kBloomUpDoubleQ, kBloomUpGeneric
};
struct BloomPassPlan {
    BloomKernel kernel;
    int grid_x, grid_y;      // blocks of 64 x 4
    DImg src, dst;
    bool vec;                // the quad kernels: 16-B stores
    float tx, ty;            // the generic kernels: 1 / source extent
};
void plan_bloom_down(const soc_img& hi, const soc_img& lo, bool force_generic, BloomPassPlan& out);
void plan_bloom_up(const soc_img& lo, const soc_img& hi, bool force_generic, BloomPassPlan& out);
int bloom_args(const soc_img& a, const soc_img& b, const char* pass);
// Below this many output pixels the 1:2 upsample runs one pixel per lane (4x the lanes of the quad kernel: small mips
// need the parallelism more than the shared window). Tuning knob: SOC_BLOOM_QUAD_MIN_PX overrides it.
long quad_min_px();

}  // namespace soc
