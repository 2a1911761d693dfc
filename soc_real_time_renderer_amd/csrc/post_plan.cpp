// post_plan.cpp — the planners of the TAA, SSAO and bloom calls: the checks in the entry points' order, the kernel form,
// the grid and the parameter block as data (post_plan.hpp). Host only: no HIP call, no image pointer dereferenced, so the
// sanitizer driver walks it and tests/test_post_plan.py compares its plans without a GPU (soc_debug_plan_post below).
// Compiled without contraction, as ssao.hip compiled the tap constants' host arithmetic.
#include "post_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace soc {

// ---- TAA ---------------------------------------------------------------------------------------------------------------
int plan_taa(const TaaCall& c, TaaPlan& out) {
    static const char* P = "soc_temporal_antialiasing";
    const soc_globals* g = c.g;
    int rc;
    if (c.tone_map) {
        static const char* PT = "soc_temporal_antialiasing_tone_mapping";
        if (!g || !c.ae) return set_error(SOC_E_INVALID_ARG, "%s: null globals / auto exposure buffer", PT);
        rc = check_img(c.output, 0, PT, "output");
        if (rc) return rc;
    }
    if (!g) return set_error(SOC_E_INVALID_ARG, "%s: null globals", P);
    const soc_img &target = c.target, &vho = c.velocity_history_out, &depth = c.depth;
    rc = check_img(target, SOC_FMT_RGBA16F, P, "target");
    if (!rc) rc = check_img(c.current_color, SOC_FMT_RGBA16F, P, "current_color");
    if (!rc) rc = check_img(c.previous_color, SOC_FMT_RGBA16F, P, "previous_color");
    if (!rc) rc = check_img(c.current_velocity, SOC_FMT_RGBA16F, P, "current_velocity");
    if (!rc) rc = check_img(c.previous_velocity, SOC_FMT_RGBA16F, P, "previous_velocity");
    if (!rc) rc = check_img(depth, SOC_FMT_D32F, P, "depth");
    if (rc) return rc;
    if (target.data == c.current_color.data || target.data == c.previous_color.data)
        return set_error(SOC_E_INVALID_ARG, "%s: target aliases an input", P);
    if (vho.data) {
        rc = check_img(vho, SOC_FMT_RGBA16F, P, "velocity_history_out");
        if (rc) return rc;
        if (vho.data == c.previous_velocity.data || vho.data == c.current_velocity.data)
            return set_error(SOC_E_INVALID_ARG, "%s: velocity_history_out aliases a velocity input", P);
        if (vho.width != c.current_velocity.width || vho.height != c.current_velocity.height)
            return set_error(SOC_E_SHAPE, "%s: velocity_history_out extent != current_velocity extent", P);
    }
    TaaParams& p = out.p;
    p.rw = recip_rn(target.width);
    p.rh = recip_rn(target.height);
    p.pox = 1.0f / (float)g->resolution[0];
    p.poy = 1.0f / (float)g->resolution[1];
    p.accum0 = fminf(0.1f, (float)g->frame_counter);
    p.swz = -16;   // XCD vertical bands of 16-tile strips: HBM traffic 1.39x -> 1.01x algorithmic
    const int W = target.width, H = target.height;
    auto same = [&](const soc_img& im) { return im.width == W && im.height == H; };
    const bool fast = W == g->resolution[0] && H == g->resolution[1] && same(c.current_color) && same(depth) &&
                      same(c.current_velocity) && W <= 8192 && H <= 8192;
    // the pair kernels address the staged images (and the depth quads through a buffer resource) with 32-bit offsets
    const bool pair = fast && W % 2 == 0 && aligned_to(target, 16) && aligned_to(c.current_color, 16) &&
                      aligned_to(c.current_velocity, 16) && aligned_to(depth, 8) && (!vho.data || aligned_to(vho, 16)) &&
                      c.previous_color.width >= 2 && c.previous_velocity.width == c.previous_color.width &&
                      c.previous_velocity.height == c.previous_color.height && buffer_range_ok(c.current_color) &&
                      buffer_range_ok(c.current_velocity) && buffer_range_ok(depth);
    // the tone map rides in the pair kernels, into an RGBA8 image of the target's extent that takes 8-B stores
    const soc_img& o = c.output;
    out.tm = c.tone_map && pair && (o.format == SOC_FMT_RGBA8_UNORM || o.format == SOC_FMT_RGBA8_SRGB) &&
             o.width == W && o.height == H && aligned_to(o, 8) && o.data != target.data;
    out.tone_mapping_pass = c.tone_map && !out.tm;   // the two passes back to back (same results)
    out.tmo = TmOut{};
    if (out.tm) {
        TmOut& tm = out.tmo;
        tm.out = dimg(o);
        tm.ae = c.ae;
        tm.srgb = o.format == SOC_FMT_RGBA8_SRGB;
        agx_matrices(g->compression, tm.p.M.m, tm.p.Minv.m);
        tm.p.linear = g->agxDs_linear_section;
        tm.p.peak = g->peak;
        tm.p.saturation = g->saturation;
        tm_params_finish(tm.p);
    }
    const soc_img* im[7] = {&target, &c.current_color, &c.previous_color, &c.current_velocity, &c.previous_velocity, &depth, &vho};
    for (int i = 0; i < 7; ++i) out.img[i] = im[i]->data ? dimg(*im[i]) : DImg{nullptr, 0, 0, 0};
    auto shape = [&](TaaKernel k, int gx, int gy, int bx, int by) {
        out.kernel = k;
        out.grid_x = gx, out.grid_y = gy, out.block_x = bx, out.block_y = by;
    };
    if (!pair) {
        shape(fast ? kTaaFast : kTaaGeneric, ceil_div(W, kTaaBX), ceil_div(H, kTaaBY), kTaaBX, kTaaBY);
        return SOC_OK;
    }
    // neighbourhood source: 4, 3 = LDS-staged tiles (default; needs a 16-B aligned depth image), 2 = halo lanes, 1 = lane
    // shifts + edge-lane loads, 0 = every lane loads its side columns (the same bits, tests/test_gpu_parity.py); without
    // the tone map only the halo form is built
    const int nbr = tuning_knob("SOC_TAA_NBR", 4);
    if ((nbr == 4 || nbr == 3) && aligned_to(depth, 16))
        shape(nbr == 4 ? kTaaLdsSf : kTaaLds, ceil_div(W / 2, kTaaPairs), ceil_div(H, kTaaLdsRows), 64, kTaaLdsRows);
    else if (!out.tm || nbr >= 2)
        shape(kTaaPair2N2, ceil_div(W / 2, 62), ceil_div(H, 4), 64, 4);
    else   // 32 x 8 lanes (64 x 8 pixels): the 3-row neighbourhood reloads 10 rows per 8 instead of 6 per 4
        shape(nbr == 0 ? kTaaPair2N0 : kTaaPair2N1, ceil_div(W / 2, 32), ceil_div(H, 8), 32, 8);
    return SOC_OK;
}

// ---- SSAO --------------------------------------------------------------------------------------------------------------
namespace {
// The tap loop's uniform constants for a depth image of W x H (sip: the sparse-inverse-projection path, whose x / y
// forms count 1/256-texel steps with the rounding's +0.5 folded into the centre).
void fold_tap_constants(SsaoParams& p, int W, int H, bool sip) {
    const float fxs = sip ? 256.0f : 1.0f;
    const float scale[3] = {0.5f * (float)W * fxs, 0.5f * (float)H * fxs, 1.0f};
    const int rows[3] = {0, 1, 3};
    for (int k = 0; k < 3; ++k)
        for (int j = 0; j < 4; ++j) p.pa[k][j] = p.proj.m[4 * j + rows[k]] * scale[k];
    const float cx0 = 0.5f * (float)(W - 1), cy0 = 0.5f * (float)(H - 1);
    const float tmax_x = (float)(W - 1) - 1.0f / 256.0f, tmax_y = (float)(H - 1) - 1.0f / 256.0f;
    p.c0x = sip ? cx0 * 256.0f + 0.5f : cx0;
    p.c0y = sip ? cy0 * 256.0f + 0.5f : cy0;
    p.tmx = sip ? tmax_x * 256.0f + 0.5f : tmax_x;
    p.tmy = sip ? tmax_y * 256.0f + 0.5f : tmax_y;
}
}  // namespace

int plan_ssao_generation(const soc_globals* g, const soc_img& depth, const soc_img& normal, const soc_img& target,
                         const float* noise_table, SsaoPlan& out, int tx, int ty) {
    if (!g) return set_error(SOC_E_INVALID_ARG, "soc_ssao_generation: null globals");
    int rc = check_img(depth, SOC_FMT_D32F, "soc_ssao_generation", "depth");
    if (!rc) rc = check_img(normal, SOC_FMT_RGBA16F, "soc_ssao_generation", "normal");
    if (!rc) rc = check_img(target, SOC_FMT_R8_UNORM, "soc_ssao_generation", "target");
    if (rc) return rc;
    if (depth.width < 2 || depth.height < 2)
        return set_error(SOC_E_SHAPE, "soc_ssao_generation: depth must be at least 2x2");
    if (!buffer_range_ok(depth))
        return set_error(SOC_E_SHAPE, "soc_ssao_generation: depth image exceeds the 2 GiB buffer-offset range");
    SsaoParams& p = out.p;
    p.inv_proj = mat4(g->camera_inverse_projection_matrix);
    p.proj = mat4(g->camera_projection_matrix);
    p.view = mat4(g->camera_view_matrix);
    p.radius = g->ssao_radius;
    p.bias = g->ssao_bias;
    p.kernel_size_f = (float)g->ssao_kernel_size;
    p.ksize = g->ssao_kernel_size < SOC_SSAO_MAX_KERNEL ? g->ssao_kernel_size : SOC_SSAO_MAX_KERNEL;
    p.noise_w = normal.width;
    p.inv_ksize = 1.0f / p.kernel_size_f;
    p.inv_radius = 1.0f / p.radius;
    p.rw = recip_rn(target.width);
    p.rh = recip_rn(target.height);
    const float *IP = g->camera_inverse_projection_matrix, *PR = g->camera_projection_matrix;
    // sparse inverse projection (the reference's perspective) whose w row stays positive over depths [-1, 1]
    const bool sip = IP[2] == 0.0f && IP[3] == 0.0f && IP[6] == 0.0f && IP[7] == 0.0f && IP[15] - IP[11] > 0.0f &&
                     IP[15] + IP[11] > 0.0f && p.radius > 0.0f && std::isfinite(p.inv_radius);
    const bool table = noise_table != nullptr, full = p.ksize == SOC_SSAO_MAX_KERNEL;
    out.depth = dimg(depth);
    out.normal = dimg(normal);
    out.target = dimg(target);
    out.noise = reinterpret_cast<const float2*>(noise_table);
    out.persp = false;
    out.early = 0;
    // default: the LDS-tiled kernel (64 x 16 pixels, 32-texel halo) in the contiguous-eighths XCD order; SOC_SSAO_TILE=0
    // selects the plain gather kernel (the same bits: tests/test_gpu_parity.py)
    if (table && sip && full && tuning_knob("SOC_SSAO_TILE", 1) != 0) {
        // SOC_SSAO_PIPE (default 1): the software-pipelined tap loop (ssao_pipe_kernel; the same bits). PERSP: the
        // projection's w row is (0, 0, -1, 0) (the reference's perspective; jitter moves only the x / y rows), so the
        // range test's sample depth comes from the tap's w'; SOC_SSAO_PIPE=2 forces the affine form
        const int pipe = tuning_knob("SOC_SSAO_PIPE", 1), early = tuning_knob("SOC_SSAO_EARLY", 2);
        out.kernel = pipe ? kSsaoPipe : kSsaoLds;
        out.persp = pipe == 1 && PR[3] == 0.0f && PR[7] == 0.0f && PR[11] == -1.0f && PR[15] == 0.0f;
        out.early = early == 1 || early == 2 ? early : 0;
        out.table = out.sip = out.full = true;
        out.grid_x = ceil_div(target.width, tx);
        out.grid_y = ceil_div(target.height, ty);
        out.block_x = tx * ty;
        p.swz = 1;
    } else {
        // a sparse inverse projection with a partial kernel and no table takes the general kernel, whose taps are in
        // texel space, not the sparse path's 1/256-texel steps
        out.kernel = kSsaoGather;
        out.table = table;
        out.sip = sip && (table || full);
        out.full = out.sip && full;
        out.grid_x = ceil_div(target.width, 32);
        out.grid_y = ceil_div(target.height, 8);
        out.block_x = kWorkgroup;
        p.swz = tuning_knob("SOC_SWZ_SSAO", -16);   // XCD vertical bands: HBM traffic 3.3x -> 1.25x algorithmic
    }
    fold_tap_constants(p, depth.width, depth.height, out.sip);
    return SOC_OK;
}

int plan_ssao_blur(const soc_img& ssao, const soc_img& target, SsaoBlurPlan& out) {
    int rc = check_img(ssao, SOC_FMT_R8_UNORM, "soc_ssao_blur", "ssao");
    if (!rc) rc = check_img(target, SOC_FMT_R8_UNORM, "soc_ssao_blur", "target");
    if (rc) return rc;
    if (ssao.data == target.data) return set_error(SOC_E_INVALID_ARG, "soc_ssao_blur: source and target alias");
    out.generic = !(ssao.width == target.width && ssao.height == target.height && ssao.width <= 8192 && ssao.height <= 8192);
    out.grid_x = ceil_div(target.width, 64);
    out.grid_y = ceil_div(target.height, 4);
    out.src = dimg(ssao);
    out.dst = dimg(target);
    out.tx = 1.0f / (float)ssao.width;
    out.ty = 1.0f / (float)ssao.height;
    return SOC_OK;
}

int check_ssao_prepare_noise(const soc_img& normal, const soc_img& target, const float* noise_table) {
    if (!noise_table) return set_error(SOC_E_INVALID_ARG, "soc_ssao_prepare_noise: null table");
    if (normal.width <= 0 || target.width <= 0 || target.height <= 0)
        return set_error(SOC_E_INVALID_ARG, "soc_ssao_prepare_noise: bad extents");
    return SOC_OK;
}

// ---- weighted bloom ----------------------------------------------------------------------------------------------------
bool bloom_fused_applicable(const soc_img& emissive, const soc_img* mips, int mip_count, const soc_img& output) {
    if (mip_count != 4 || output.width != emissive.width || output.height != emissive.height) return false;
    if (emissive.width > 8192 || emissive.height > 8192) return false;
    if (mips[0].width != emissive.width || mips[0].height != emissive.height) return false;
    for (int i = 1; i < 4; ++i)
        if (mips[i - 1].width != 2 * mips[i].width || mips[i - 1].height != 2 * mips[i].height || mips[i].width < 2 ||
            mips[i].height < 2)
            return false;
    return true;
}

bool bloom_sparse_applicable() {
    return tuning_knob("SOC_BLOOM_SPARSE", 1) != 0 && tuning_knob("SOC_BLOOM_ZERO_SKIP", 1) != 0 &&
           tuning_knob("SOC_BLOOM_UP10_REG", 1) != 0;
}

int check_bloom_weighted_stage(const soc_img& emissive, const soc_img* mips, int mip_count, const soc_img& output, int stage) {
    static const char* P = "soc_bloom_weighted_stage";
    if (!mips) return set_error(SOC_E_INVALID_ARG, "%s: null mips", P);
    if (stage < 0 || stage > 4) return set_error(SOC_E_INVALID_ARG, "%s: stage %d not in 0..4", P, stage);
    int rc = check_img(emissive, SOC_FMT_RGBA16F, P, "emissive");
    if (!rc) rc = check_img(output, SOC_FMT_RGBA16F, P, "output");
    for (int i = 0; !rc && i < mip_count; ++i) rc = check_img(mips[i], SOC_FMT_RGBA16F, P, "mip");
    if (rc) return rc;
    if (!bloom_fused_applicable(emissive, mips, mip_count, output))
        return set_error(SOC_E_UNSUPPORTED, "%s: needs 4 mips halving exactly from the emissive extent (<= 8192)", P);
    if ((stage == 0 || stage == 4) && output.data == mips[1].data)
        return set_error(SOC_E_INVALID_ARG, "%s: output aliases mip 1", P);
    return SOC_OK;
}

int plan_bloom_weighted(const soc_img& emissive, const soc_img* mips, const soc_img& output, int stage, bool sparse_output,
                        const int resident[6], BloomwPlan& out, int rows) {
    const bool last = stage == 0 || stage == 4;
    if (last && sparse_output && !bloom_sparse_applicable())
        return set_error(SOC_E_INVALID_ARG, "bloom_weighted: the sparse output needs the register-form last stage and the zero skip");
    const DImg E = dimg(emissive), M1 = dimg(mips[1]), M3 = dimg(mips[3]), O = dimg(output), none{nullptr, 0, 0, 0};
    const int swz = 1;   // XCD-aware order: halo re-reads served by L2 (2.0x -> 1.0x HBM traffic)
    // all-zero tiles / rows skip their filters (bloomw_down01p, bloomw_up10r): 0 = every tile filtered, the same bits
    const bool zero_skip = tuning_knob("SOC_BLOOM_ZERO_SKIP", 1) != 0;
    const bool up_sep = tuning_knob("SOC_BLOOM_UP_SEP", 1) != 0;
    const int w2 = mips[2].width, h2 = mips[2].height;
    out.n = 0;
    auto add = [&](BloomwKernel k, int f0, int f1, int gx, int gy, DImg src, DImg dst, DImg m3, int a0, int a1, int a2, int a3) {
        out.st[out.n++] = BloomwStage{k, f0, f1, gx, gy, src, dst, m3, {a0, a1, a2, a3}};
    };
    if (stage == 0 || stage == 1) {
        // persistent: one resident set of workgroups (a multiple of 8, so a workgroup's tiles stay on its XCD)
        const int knob = tuning_knob("SOC_BLOOM_W1_REG", 1), mode = knob == 2 || knob == 1 ? knob : 0;
        if (!resident) return set_error(SOC_E_INVALID_ARG, "bloom_weighted: null resident sets");
        const int ntx = ceil_div(mips[1].width, w1_ow(mode)), nty = ceil_div(mips[1].height, w1_oh(mode));
        const int grid = std::max(8, (std::min(ntx * nty, resident[mode * 2 + zero_skip]) / 8) * 8);
        add(kBwDown01p, mode, zero_skip, grid, 1, E, M1, none, ntx, nty, 0, 0);
    }
    if (stage == 0 || stage == 2)
        add(kBwDown23, tuning_knob("SOC_BLOOM_W2_REG", 1) != 0, 0, ceil_div(mips[3].width, W2_OW), ceil_div(mips[3].height, W2_OH),
            M1, M3, none, w2, h2, swz, 0);
    if (stage == 0 || stage == 3) {
        const int gx = ceil_div(mips[1].width, U_OW), gy = ceil_div(mips[1].height, U_OH), vec = aligned_to(mips[1], 16);
        if (up_sep) add(kBwUp32s, tuning_knob("SOC_BLOOM_W3_RUNS", 1) != 0, 0, gx, gy, M3, M1, none, w2, h2, vec, swz);
        else add(kBwUp32, 0, 0, gx, gy, M3, M1, none, w2, h2, vec, swz);
    }
    if (last) {
        const int gx = ceil_div(output.width, U_OW), gy = ceil_div(output.height, U_OH), vec = aligned_to(output, 16);
        if (tuning_knob("SOC_BLOOM_UP10_REG", 1)) {
            // sparse: proven-zero strips store nothing (bloom_sparse_applicable held: zero_skip and this form)
            const int nwx = ceil_div(output.width, R_OW), nwaves = nwx * ceil_div(output.height, rows);
            add(kBwUp10r, zero_skip || sparse_output, sparse_output, ceil_div(nwaves, kWorkgroup / 64), 1, M1, O, M3, nwx, nwaves, 0, 0);
        } else if (up_sep)
            add(kBwUp10s, 0, 0, gx, gy, M1, O, none, vec, swz, zero_skip, 0);
        else
            add(kBwUp10, 0, 0, gx, gy, M1, O, none, vec, swz, 0, 0);
    }
    return SOC_OK;
}

// ---- per-pass bloom ----------------------------------------------------------------------------------------------------
long quad_min_px() {
    static const long v = [] {
        const char* e = getenv("SOC_BLOOM_QUAD_MIN_PX");
        return e ? atol(e) : 1L << 20;
    }();
    return v;
}

namespace {
constexpr int kFastMax = 8192;
// same extent, the exact 2:1 ratio, or neither: 0, 1, 2
int bloom_ratio(const soc_img& hi, const soc_img& lo, bool force_generic) {
    if (force_generic || hi.width > kFastMax || hi.height > kFastMax) return 2;
    if (hi.width == lo.width && hi.height == lo.height) return 0;
    return hi.width == 2 * lo.width && hi.height == 2 * lo.height ? 1 : 2;
}
}  // namespace

void plan_bloom_down(const soc_img& hi, const soc_img& lo, bool force_generic, BloomPassPlan& out) {
    const int ratio = bloom_ratio(hi, lo, force_generic);
    const int half = ratio == 0 ? 2 : 1;   // the quad kernel: 2 x 2 outputs per lane
    out = BloomPassPlan{ratio == 0 ? kBloomDownSameQ : ratio == 1 ? kBloomDownHalfW : kBloomDownGeneric,
                        (int)ceil_div(ceil_div(lo.width, half), kBloomBX), (int)ceil_div(ceil_div(lo.height, half), kBloomBY),
                        dimg(hi), dimg(lo), aligned_to(lo, 16), 1.0f / (float)hi.width, 1.0f / (float)hi.height};
}

void plan_bloom_up(const soc_img& lo, const soc_img& hi, bool force_generic, BloomPassPlan& out) {
    const int ratio = bloom_ratio(hi, lo, force_generic);
    const bool quad = ratio == 0 || (ratio == 1 && (long)hi.width * hi.height >= quad_min_px());
    const int half = quad ? 2 : 1;
    out = BloomPassPlan{ratio == 0 ? kBloomUpSameQ : ratio == 2 ? kBloomUpGeneric : quad ? kBloomUpDoubleQ : kBloomUpDouble,
                        (int)ceil_div(ceil_div(hi.width, half), kBloomBX), (int)ceil_div(ceil_div(hi.height, half), kBloomBY),
                        dimg(lo), dimg(hi), aligned_to(hi, 16), 1.0f / (float)lo.width, 1.0f / (float)lo.height};
}

int bloom_args(const soc_img& a, const soc_img& b, const char* pass) {
    int rc = check_img(a, SOC_FMT_RGBA16F, pass, "source");
    if (rc) return rc;
    rc = check_img(b, SOC_FMT_RGBA16F, pass, "target");
    if (rc) return rc;
    if (a.data == b.data) return set_error(SOC_E_INVALID_ARG, "%s: source and target alias", pass);
    return SOC_OK;
}

}  // namespace soc

using namespace soc;

namespace {
void add(std::string& out, const char* fmt, ...) {
    char line[1024];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(line, sizeof line, fmt, ap);
    va_end(ap);
    out += line;
}
void add_bits(std::string& out, const float* v, int n) {
    for (int i = 0; i < n; ++i) {
        uint32_t u;
        memcpy(&u, v + i, sizeof u);
        add(out, "%s%08x", i ? "," : "", u);
    }
}
void add_kernel(std::string& out, const char* name, const char* form, int gx, int gy, int bx, int by) {
    add(out, "kernel\t%s\t%s\t%dx%dx1\t%dx%dx1\t", name, form, gx, gy, bx, by);
}
}  // namespace

// Test hook (not in the public header): the plan of a TAA, SSAO or bloom call as text, without a HIP call. pass: 0
// soc_temporal_antialiasing (images: target, colour, history, velocity, velocity history, depth, velocity_history_out),
// 1 soc_temporal_antialiasing_tone_mapping (an eighth image: output; aux: the auto-exposure buffer), 2 soc_ssao_generation
// (depth, normal, target; aux: the noise table), 3 soc_ssao_blur (ssao, target), 4 soc_ssao_prepare_noise (normal, target;
// aux: the table), 5 soc_bloom_weighted_stage (emissive, output, then the mips, none: a null pointer; arg: the stage, + 256 for the render
// graph's sparse-output call, which skips the entry point's checks; resident: bloomw_down01p's six resident sets),
// 6 / 7 soc_bloom_downsample / soc_bloom_upsample (source, target; arg: 1 forces the generic kernel, as
// soc_debug_bloom_generic). A header line with the parameter block's scalars (floats as bit patterns), then
// "kernel<TAB>name<TAB>form<TAB>grid<TAB>block<TAB>scalar arguments" per launch and "pass<TAB>tone_mapping" for a following
// tone-map pass. Returns the text's length (truncated to cap - 1 characters in `buf`), or the call's error code.
extern "C" int64_t soc_debug_plan_post(int32_t pass, const soc_globals* g, const soc_img* images, int32_t n_images, const void* aux,
                                       int32_t arg, const int32_t* resident, char* buf, size_t cap) {
    static const int need[8] = {7, 8, 3, 2, 2, 2, 2, 2};
    if (pass < 0 || pass > 7 || !images || n_images < need[pass])
        return set_error(SOC_E_INVALID_ARG, "soc_debug_plan_post: pass %d needs %d images", pass, pass >= 0 && pass <= 7 ? need[pass] : 0);
    std::string out;
    if (pass <= 1) {
        const TaaCall c = {g, images[0], images[1], images[2], images[3], images[4], images[5], images[6], pass == 1,
                           static_cast<const soc_auto_exposure*>(aux), pass == 1 ? images[7] : soc_img{}};
        TaaPlan pl;
        const int rc = plan_taa(c, pl);
        if (rc) return rc;
        add(out, "taa\t%d\t%d\tswz=%d\tp=", pl.img[0].w, pl.img[0].h, pl.p.swz);
        add_bits(out, &pl.p.rw, 5);
        if (pl.tm) {
            add(out, "\ttm=%d,%dx%d,", pl.tmo.srgb, pl.tmo.out.w, pl.tmo.out.h);
            add_bits(out, pl.tmo.p.M.m, 9);
            add(out, ",");
            add_bits(out, pl.tmo.p.Minv.m, 9);
            add(out, ",");
            add_bits(out, &pl.tmo.p.linear, 6);
        }
        static const char* names[kTaaKernels] = {"taa_lds", "taa_lds", "taa_pair2", "taa_pair2", "taa_pair2", "taa_fast", "taa_generic"};
        char form[32] = "-";
        if (pl.kernel <= kTaaLds) std::snprintf(form, sizeof form, "tm=%d sf=%d", pl.tm, pl.kernel == kTaaLdsSf);
        else if (pl.kernel <= kTaaPair2N2) std::snprintf(form, sizeof form, "tm=%d nbr=%d", pl.tm, pl.kernel - kTaaPair2N0);
        add(out, "\n");
        add_kernel(out, names[pl.kernel], form, pl.grid_x, pl.grid_y, pl.block_x, pl.block_y);
        add(out, "vel_out=%d\n", pl.img[6].data != nullptr);
        if (pl.tone_mapping_pass) out += "pass\ttone_mapping\n";
    } else if (pass == 2) {
        SsaoPlan pl;
        const int rc = plan_ssao_generation(g, images[0], images[1], images[2], static_cast<const float*>(aux), pl);
        if (rc) return rc;
        const SsaoParams& p = pl.p;
        add(out, "ssao_generation\t%d\t%d\ttable=%d\tksize=%d\tnoise_w=%d\tswz=%d\tp=", pl.target.w, pl.target.h, pl.noise != nullptr,
            p.ksize, p.noise_w, p.swz);
        add_bits(out, &p.radius, 3);
        add(out, ",");
        add_bits(out, &p.rw, 2);
        add(out, "\tpa=");
        add_bits(out, &p.pa[0][0], 12);
        add(out, "\tc=");
        add_bits(out, &p.c0x, 6);
        add(out, "\n");
        char form[48];
        if (pl.kernel == kSsaoPipe) std::snprintf(form, sizeof form, "persp=%d", pl.persp);
        else if (pl.kernel == kSsaoLds) std::snprintf(form, sizeof form, "early=%d", pl.early);
        else std::snprintf(form, sizeof form, "table=%d sip=%d full=%d", pl.table, pl.sip, pl.full);
        static const char* names[] = {"ssao_pipe_kernel", "ssao_lds_kernel", "ssao_kernel"};
        add_kernel(out, names[pl.kernel], form, pl.grid_x, pl.grid_y, pl.block_x, 1);
        add(out, "-\n");
    } else if (pass == 3) {
        SsaoBlurPlan pl;
        const int rc = plan_ssao_blur(images[0], images[1], pl);
        if (rc) return rc;
        add(out, "ssao_blur\t%d\t%d\n", pl.dst.w, pl.dst.h);
        add_kernel(out, pl.generic ? "ssao_blur_generic" : "ssao_blur_kernel", "-", pl.grid_x, pl.grid_y, 64, 4);
        if (pl.generic) add_bits(out, &pl.tx, 2);
        else add(out, "-");
        add(out, "\n");
    } else if (pass == 4) {
        const int rc = check_ssao_prepare_noise(images[0], images[1], static_cast<const float*>(aux));
        if (rc) return rc;
        add(out, "ssao_prepare_noise\t%d\t%d\n", images[1].width, images[1].height);
        add_kernel(out, "ssao_noise_kernel", "-", ceil_div(images[1].width, 64), ceil_div(images[1].height, 4), 64, 4);
        add(out, "%d,%d,%d\n", images[1].width, images[1].height, images[0].width);
    } else if (pass == 5) {
        const int stage = arg & 255;
        const bool sparse = (arg & 256) != 0;
        const soc_img* mips = n_images > 2 ? images + 2 : nullptr;
        int rc = sparse ? (n_images < 6 ? set_error(SOC_E_INVALID_ARG, "soc_debug_plan_post: the sparse call needs 4 mips") : SOC_OK)
                        : check_bloom_weighted_stage(images[0], mips, n_images - 2, images[1], stage);
        BloomwPlan pl;
        if (!rc) rc = plan_bloom_weighted(images[0], mips, images[1], stage, sparse, resident, pl);
        if (rc) return rc;
        add(out, "bloom_weighted\tstage=%d\tsparse=%d\n", stage, sparse);
        static const char* names[] = {"bloomw_down01p", "bloomw_down23", "bloomw_up32s", "bloomw_up32", "bloomw_up10r", "bloomw_up10s", "bloomw_up10"};
        static const char* forms[] = {"mode=%d zs=%d", "reg=%d", "runs=%d", "-", "zs=%d sparse=%d", "-", "-"};
        for (int i = 0; i < pl.n; ++i) {
            const BloomwStage& s = pl.st[i];
            char form[32];
            std::snprintf(form, sizeof form, forms[s.kernel], s.f0, s.f1);
            add_kernel(out, names[s.kernel], form, s.grid_x, s.grid_y, kWorkgroup, 1);
            add(out, "%d,%d,%d,%d\tsrc=%dx%d\tdst=%dx%d\tm3=%dx%d\n", s.a[0], s.a[1], s.a[2], s.a[3], s.src.w, s.src.h, s.dst.w, s.dst.h,
                s.m3.w, s.m3.h);
        }
    } else {
        const int rc = bloom_args(images[0], images[1], arg ? "soc_debug_bloom_generic" : pass == 6 ? "soc_bloom_downsample" : "soc_bloom_upsample");
        if (rc) return rc;
        BloomPassPlan pl;
        if (pass == 6) plan_bloom_down(images[0], images[1], arg != 0, pl);
        else plan_bloom_up(images[0], images[1], arg != 0, pl);
        add(out, "%s\t%d\t%d\n", pass == 6 ? "bloom_down" : "bloom_up", pl.dst.w, pl.dst.h);
        static const char* names[] = {"bloom_down_same_q", "bloom_down_half_w", "bloom_down_generic", "bloom_up_same_q", "bloom_up_double",
                                      "bloom_up_double_q", "bloom_up_generic"};
        const bool quad = pl.kernel == kBloomDownSameQ || pl.kernel == kBloomUpSameQ || pl.kernel == kBloomUpDoubleQ;
        const bool generic = pl.kernel == kBloomDownGeneric || pl.kernel == kBloomUpGeneric;
        add_kernel(out, names[pl.kernel], "-", pl.grid_x, pl.grid_y, kBloomBX, kBloomBY);
        if (quad) add(out, "vec=%d", pl.vec);
        else if (generic) add_bits(out, &pl.tx, 2);
        else add(out, "-");
        add(out, "\n");
    }
    return copy_text(out, buf, cap);
}
