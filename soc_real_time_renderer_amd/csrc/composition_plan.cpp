// composition_plan.cpp — the planner of a Composition call: the argument checks in the entry points' order, CompParams
// and its bounded / cascaded extensions, the pair-path predicate, the fused histogram's fallback, and from them the
// kernel form and grid that composition.hip's issue_composition launches; the same for SkyCompose. Host only: no HIP
// call, no image pointer dereferenced (tests/test_composition_plan.py runs it without a GPU through
// soc_debug_plan_composition). Compiled with composition.hip's flags: bin_fast_params and recip_rn are inline host
// arithmetic, and the kernels take their results bit for bit.
#include "composition_plan.hpp"

#include <cstring>

namespace soc {
namespace {

bool aligned16(const soc_img& im) {
    return (reinterpret_cast<uintptr_t>(im.data) & 15u) == 0 && (im.pitch_bytes & 15) == 0;
}

// The cascaded instantiations' parameter block: the record's matrices (and the camera's inverses) widened to fp64, the
// factors as they are (the unused entries repeat the last cascade) and +inf for the splits that do not exist.
void cascaded_params(CompParamsCascaded& pc, const soc_sun_cascades& cs, int W, int H) {
    pc.count = cs.count;
    pc.S = cs.map_size;
    for (int i = 0; i < 16; ++i) {
        pc.inv_proj_d.m[i] = (double)pc.inv_proj.m[i];
        pc.inv_view_d.m[i] = (double)pc.inv_view.m[i];
    }
    pc.rw_d = 1.0 / (double)W;
    pc.rh_d = 1.0 / (double)H;
    for (int k = 0; k < SOC_MAX_SUN_CASCADES; ++k) {
        const int c = k < cs.count ? k : cs.count - 1;
        for (int i = 0; i < 16; ++i) pc.pv[k].m[i] = (double)cs.projection_view[c][i];
        pc.ef[k] = cs.exponential_factor[c];
        if (k < SOC_MAX_SUN_CASCADES - 1) pc.split[k] = k < cs.count - 1 ? cs.split_depth[k] : __builtin_inff();
    }
}

// the fused histogram's part of the parameter block (composition_pair<true, ...>, sky_compose_pair)
void histogram_params(CompParams& p, const soc_globals* g, uint32_t* scratch) {
    p.bins = scratch;
    p.lmin = g->log_min_luminance;
    p.lrange = g->log_max_luminance - g->log_min_luminance;
    p.bf = bin_fast_params(p.lmin, p.lrange);
}

}  // namespace

CompositionCall composition_call(const soc_globals* g, const soc_globals* d_globals, const soc_img (&im)[8]) {
    CompositionCall c = {};
    c.g = g;
    c.d_globals = d_globals;
    c.target = im[0];
    c.albedo = im[1];
    c.emissive = im[2];
    c.normal = im[3];
    c.depth = im[4];
    c.ssao = im[5];
    c.shadow = im[6];
    c.clouds = im[7];
    return c;
}

bool composition_pair_path(const CompositionCall& c) {
    const int W = c.target.width, H = c.target.height;
    auto same = [&](const soc_img& im) { return im.width == W && im.height == H; };
    return same(c.albedo) && same(c.emissive) && same(c.normal) && same(c.depth) && same(c.clouds) && (W % 2 == 0) &&
           W <= 8192 && H <= 8192 && aligned16(c.target) && aligned16(c.albedo) && aligned16(c.emissive) &&
           aligned16(c.normal) && (reinterpret_cast<uintptr_t>(c.depth.data) & 7u) == 0 && (c.depth.pitch_bytes & 7) == 0;
}

bool composition_pair_applicable(const soc_globals* g, const soc_img& target, const soc_img& albedo, const soc_img& emissive,
                                 const soc_img& normal, const soc_img& depth, const soc_img& clouds) {
    CompositionCall c = {};
    c.target = target;
    c.albedo = albedo;
    c.emissive = emissive;
    c.normal = normal;
    c.depth = depth;
    c.clouds = clouds;
    return g && composition_pair_path(c) && target.width == g->resolution[0] && target.height == g->resolution[1];
}

int plan_composition(const CompositionCall& c, CompositionPlan& out) {
    static const char* P = "soc_composition";
    out = CompositionPlan{};
    const soc_globals* g = c.g;
    if (c.histogram && (!g || !c.ae || !c.scratch))
        return set_error(SOC_E_INVALID_ARG, "soc_composition_luminance_histogram: null globals / auto exposure / scratch");
    if (!g) return set_error(SOC_E_INVALID_ARG, "%s: null globals", P);
    const LightBoundsCall* bc = c.bounds;
    int rc = SOC_OK;
    if (c.cascaded) {   // the record and its atlas first, so that the message names the cascades' field
        rc = check_sun_cascades(c.cascades, &c.shadow, P);
        if (rc) return rc;
        if (bc) return set_error(SOC_E_UNSUPPORTED, "%s: sun cascades with bounded lights are not supported", P);
        if (c.bloom_mip1) return set_error(SOC_E_UNSUPPORTED, "%s: sun cascades with the in-kernel bloom are not supported", P);
        if (c.bloom_mip3) return set_error(SOC_E_UNSUPPORTED, "%s: sun cascades with the bloom's zero cells are not supported", P);
    }
    rc = check_img(c.target, SOC_FMT_RGBA16F, P, "target");
    if (!rc) rc = check_img(c.albedo, SOC_FMT_RGBA16F, P, "albedo");
    if (!rc) rc = check_img(c.emissive, SOC_FMT_RGBA16F, P, "emissive");
    if (!rc) rc = check_img(c.normal, SOC_FMT_RGBA16F, P, "normal");
    if (!rc) rc = check_img(c.depth, SOC_FMT_D32F, P, "depth");
    if (!rc) rc = check_img(c.ssao, SOC_FMT_R8_UNORM, P, "ssao");
    if (!rc) rc = check_img(c.shadow, SOC_FMT_D32F, P, "shadow");
    if (!rc) rc = check_img(c.clouds, SOC_FMT_RGBA8_UNORM, P, "clouds");
    if (rc) return rc;
    CompParams& p = out.p;
    p.inv_proj = mat4(g->camera_inverse_projection_matrix);
    p.inv_view = mat4(g->camera_inverse_view_matrix);
    mat4_mul_host(p.sun_pv.m, g->sun_info.projection_matrix, g->sun_info.view_matrix);
    {
        float t[16];
        mat4_mul_host(t, p.sun_pv.m, g->camera_inverse_view_matrix);
        mat4_mul_host(p.sun_clip.m, t, g->camera_inverse_projection_matrix);
    }
    for (int i = 0; i < 3; ++i) {
        p.sun_dir[i] = g->sun_info.direction[i];
        p.ambient[i] = g->ambient[i];
        p.cam[i] = g->camera_position[i];
    }
    p.ef = g->sun_info.exponential_factor;
    p.df = g->sun_info.darkening_factor;
    p.emissive_strength = g->emissive_bloom_strength;
    p.ao_strength = g->ambient_occlussion_strength;
    p.npl = g->point_light_count < SOC_MAX_POINT_LIGHTS ? g->point_light_count : SOC_MAX_POINT_LIGHTS;
    p.nsl = g->spot_light_count < SOC_MAX_SPOT_LIGHTS ? g->spot_light_count : SOC_MAX_SPOT_LIGHTS;
    p.dg = c.d_globals;
    p.swz = 0;   // row-major (the strip order measured 66 -> 77 us)
    p.rw = recip_rn(c.target.width);
    p.rh = recip_rn(c.target.height);
    p.bloom_zero_skip = tuning_knob("SOC_BLOOM_ZERO_SKIP", 1) != 0;
    const bool lights = (p.npl | p.nsl) != 0;
    if (lights && !c.d_globals)
        return set_error(SOC_E_INVALID_ARG, "%s: frame has lights but no device globals (soc_upload_globals)", P);
    if (bc && !bc->d_bounds) return set_error(SOC_E_INVALID_ARG, "%s: bounded call without light bounds (soc_upload_light_bounds)", P);
    if (bc && (bc->flags & ~(uint32_t)SOC_LIGHTS_CULL)) return set_error(SOC_E_INVALID_ARG, "%s: unknown light flags %u", P, bc->flags);

    const int W = c.target.width, H = c.target.height;
    const bool pair = composition_pair_path(c);
    // the histogram is fused into the pair kernel at the globals' resolution; any other call takes the two passes back to
    // back (same results), which the renderer-only forms cannot
    bool hist = c.histogram;
    if (hist && !(pair && W == g->resolution[0] && H == g->resolution[1])) {
        if (c.bloom_mip3) return set_error(SOC_E_SHAPE, "composition: the bloom's zero cells need the pair path");
        if (c.bloom_mip1) return set_error(SOC_E_SHAPE, "composition: the in-kernel bloom needs the pair path");
        if (c.sky_external) return set_error(SOC_E_INVALID_ARG, "composition: sky_external needs the pair path");
        hist = false;
        out.histogram_pass = true;
    }
    if (c.sky_external && !hist) return set_error(SOC_E_INVALID_ARG, "%s: sky_external needs the fused histogram", P);
    if (c.bloom_mip1) {
        rc = check_img(*c.bloom_mip1, SOC_FMT_RGBA16F, P, "bloom mip1");
        if (rc) return rc;
        if (!hist || !pair || c.bloom_mip1->width * 2 != W || c.bloom_mip1->height * 2 != H)
            return set_error(SOC_E_SHAPE, "%s: the in-kernel bloom needs the fused histogram's pair path and mip1 = W/2 x H/2", P);
        out.mip1 = dimg(*c.bloom_mip1);
    }
    if (c.bloom_mip3) {
        rc = check_img(*c.bloom_mip3, SOC_FMT_RGBA16F, P, "bloom mip3");
        if (rc) return rc;
        if (!hist || !pair || c.bloom_mip3->width * 8 != W || c.bloom_mip3->height * 8 != H)
            return set_error(SOC_E_SHAPE, "%s: the bloom's zero cells need the fused histogram's pair path and mip3 = W/8 x H/8", P);
        out.mip3 = dimg(*c.bloom_mip3);
    }
    p.bloom_sparse = c.bloom_mip3 != nullptr;
    if (hist) {
        histogram_params(p, g, c.scratch);
        p.sky_external = c.sky_external ? 1 : 0;
        out.fold = c.fold;
        out.scratch = c.scratch;
        out.bins = c.ae->histogram_buckets;
    }
    const soc_img* imgs[8] = {&c.target, &c.albedo, &c.emissive, &c.normal, &c.depth, &c.ssao, &c.shadow, &c.clouds};
    for (int i = 0; i < 8; ++i) out.img[i] = dimg(*imgs[i]);
    // bounded lights: a frame without lights has nothing to bound and takes the unbounded kernels
    const bool bounded = bc && lights;
    if (bounded) out.la = LightArgs{static_cast<const LightBoundsDev*>(bc->d_bounds), bc->d_shaded_pairs};
    if (c.cascaded) cascaded_params(out.p, *c.cascades, W, H);
    if (!pair) {
        out.kernel = c.cascaded ? kCompGenericCascaded : bounded ? kCompGenericBounded : kCompGeneric;
        out.grid_x = ceil_div(W, kGenericBlockX);
        out.grid_y = ceil_div(H, kGenericBlockY);
        out.block_x = kGenericBlockX;
        out.block_y = kGenericBlockY;
        return SOC_OK;
    }
    // The pair kernel's form. The in-kernel bloom (bl) and the zero cells as a template parameter (sp: the forms with
    // lights or bl; the others read p.bloom_sparse) are the render graph's. The lights forms are always nt = 0; without
    // lights a cascaded or in-kernel-bloom form is always nt = 7, and the others follow the knobs: SOC_COMP_NT (default 3:
    // non-temporal G-buffer loads and colour store, measured at 4K 71.5 -> 68 us; 0: the default cache policy, for the
    // variant-identity test) and, under it, SOC_COMP_AOP (default 1: nt = 7, both AO taps of a pair as one load per row;
    // 0: 4 byte loads per pixel after the depth test).
    PairForm& f = out.form;
    f.hist = hist;
    f.lights = lights;
    f.bl = c.bloom_mip1 != nullptr;
    f.sp = c.bloom_mip3 != nullptr && (lights || f.bl);
    f.cs = c.cascaded;
    if (bounded) f.lb = kLbBounded | ((bc->flags & SOC_LIGHTS_CULL) ? kLbCull : 0) | (bc->d_shaded_pairs ? kLbCount : 0);
    if ((f.lb & kLbCount) && (f.bl || f.sp))
        return set_error(SOC_E_INVALID_ARG, "%s: the shaded-pairs counter is the stand-alone calls'", P);
    if (lights) f.nt = 0;
    else if (f.cs || f.bl) f.nt = 7;
    else if (tuning_knob("SOC_COMP_NT", 3) != 3) f.nt = 0;
    else f.nt = tuning_knob("SOC_COMP_AOP", 1) != 0 ? 7 : 3;
    out.kernel = kCompPair;
    out.grid_x = ceil_div(W, 32);
    out.grid_y = ceil_div(H, 16);
    out.block_x = kWorkgroup;
    out.block_y = 1;
    return SOC_OK;
}

int plan_sky_compose(const soc_globals* g, const soc_img& target, const soc_img& depth, const soc_img& clouds,
                     uint32_t* scratch, SkyComposePlan& out) {
    out = SkyComposePlan{};
    if (!g || !scratch) return set_error(SOC_E_INVALID_ARG, "sky compose: null globals / scratch");
    int rc = check_img(target, SOC_FMT_RGBA16F, "sky compose", "target");
    if (!rc) rc = check_img(depth, SOC_FMT_D32F, "sky compose", "depth");
    if (!rc) rc = check_img(clouds, SOC_FMT_RGBA8_UNORM, "sky compose", "clouds");
    if (rc) return rc;
    histogram_params(out.p, g, scratch);
    out.target = dimg(target);
    out.depth = dimg(depth);
    out.clouds = dimg(clouds);
    out.grid_x = ceil_div(target.width, 32);
    out.grid_y = ceil_div(target.height, 16);
    out.pair_load = (clouds.pitch_bytes % 8) == 0 && (reinterpret_cast<uintptr_t>(clouds.data) % 8) == 0 &&
                    tuning_knob("SOC_SKY_COMPOSE_PAIR_LOAD", 1);
    return SOC_OK;
}

}  // namespace soc

using namespace soc;

// Test hook (not in the public header): the plan of a Composition call as text, without a HIP call. `what`: 1 a
// *_luminance_histogram call (ae, scratch), 2 with its fold, 4 sky_external, 8 bounded (d_bounds, light_flags, d_shaded), 16 a
// cascaded entry point (cascades), 32 SkyCompose instead (images[0], [4] and [7], scratch). images: target, albedo,
// emissive, normal, depth, ssao, shadow, clouds. A header line "composition<TAB>pair|generic<TAB>W<TAB>H" with the
// parameter block's scalars and the bit patterns of its host arithmetic (the histogram's only under the fused histogram,
// the cascades' only in a cascaded call), then "kernel<TAB>name<TAB>form<TAB>grid<TAB>block<TAB>mip1, mip3 extents, bounds,
// counter" per launch and "pass<TAB>generate_luminance_histogram" for a following histogram pass. Returns the text's
// length (truncated to cap - 1 characters in `buf`), or the call's error code.
extern "C" int64_t soc_debug_plan_composition(const soc_globals* g, const soc_globals* d_globals, const soc_img* images,
                                              uint32_t what, soc_auto_exposure* ae, uint32_t* scratch, const soc_img* mip1,
                                              const soc_img* mip3, const void* d_bounds, uint32_t light_flags,
                                              uint32_t* d_shaded, const soc_sun_cascades* cascades, char* buf, size_t cap) {
    if (!images) return set_error(SOC_E_INVALID_ARG, "soc_debug_plan_composition: null images");
    std::string out;
    char line[1024];
    auto bits = [](float v) {
        uint32_t u;
        memcpy(&u, &v, sizeof u);
        return u;
    };
    auto histogram = [&](const CompParams& p) {
        std::snprintf(line, sizeof line, "\thist=%08x,%08x,%08x,%08x,%08x,%u", bits(p.lmin), bits(p.lrange), bits(p.bf.lmin),
                      bits(p.bf.rlr), bits(p.bf.eps), p.bf.zero);
        out += line;
    };
    if (what & 32u) {
        SkyComposePlan pl;
        const int rc = plan_sky_compose(g, images[0], images[4], images[7], scratch, pl);
        if (rc) return rc;
        std::snprintf(line, sizeof line, "sky_compose\t%d\t%d", pl.target.w, pl.target.h);
        out += line;
        histogram(pl.p);
        std::snprintf(line, sizeof line, "\nkernel\tsky_compose_pair\tcp=%d\t%dx%dx1\t%dx1x1\n", pl.pair_load, pl.grid_x, pl.grid_y, kWorkgroup);
        out += line;
        return copy_text(out, buf, cap);
    }
    const LightBoundsCall bc = {d_bounds, light_flags, d_shaded};
    CompositionCall c = composition_call(g, d_globals, *reinterpret_cast<const soc_img(*)[8]>(images));   // the caller's eight
    c.histogram = (what & 1u) != 0;
    c.ae = ae;
    c.scratch = scratch;
    c.fold = (what & 2u) != 0;
    c.sky_external = (what & 4u) != 0;
    c.bloom_mip1 = mip1;
    c.bloom_mip3 = mip3;
    c.bounds = (what & 8u) ? &bc : nullptr;
    c.cascades = cascades;
    c.cascaded = (what & 16u) != 0;
    CompositionPlan pl;
    const int rc = plan_composition(c, pl);
    if (rc) return rc;
    const CompParamsCascaded& p = pl.p;
    std::snprintf(line, sizeof line, "composition\t%s\t%d\t%d\tnpl=%u\tnsl=%u\tsky_external=%d\tzero_skip=%d\tsparse=%d\tbins=%d\t"
                  "rw=%08x\trh=%08x\tsun_clip=", pl.kernel == kCompPair ? "pair" : "generic", pl.img[0].w, pl.img[0].h, p.npl,
                  p.nsl, p.sky_external, p.bloom_zero_skip, p.bloom_sparse, p.bins != nullptr, bits(p.rw), bits(p.rh));
    out += line;
    for (int i = 0; i < 16; ++i) {
        std::snprintf(line, sizeof line, "%s%08x", i ? "," : "", bits(p.sun_clip.m[i]));
        out += line;
    }
    if (p.bins) histogram(p);
    if (c.cascaded) {
        std::snprintf(line, sizeof line, "\tcascades=%d,%d:%08x,%08x,%08x;%08x,%08x,%08x,%08x", p.count, p.S, bits(p.split[0]),
                      bits(p.split[1]), bits(p.split[2]), bits(p.ef[0]), bits(p.ef[1]), bits(p.ef[2]), bits(p.ef[3]));
        out += line;
    }
    const PairForm& f = pl.form;
    char form[96] = "-";
    if (pl.kernel == kCompPair)
        std::snprintf(form, sizeof form, "hist=%d lights=%d nt=%d bl=%d sp=%d lb=%d cs=%d", f.hist, f.lights, f.nt, f.bl, f.sp, f.lb, f.cs);
    static const char* names[] = {"composition_pair", "composition_generic", "composition_generic_bounded", "composition_generic_cascaded"};
    std::snprintf(line, sizeof line, "\nkernel\t%s\t%s\t%dx%dx1\t%dx%dx1\tmip1=%dx%d\tmip3=%dx%d\tbounds=%d\tcounter=%d\n", names[pl.kernel],
                  form, pl.grid_x, pl.grid_y, pl.block_x, pl.block_y, pl.mip1.w, pl.mip1.h, pl.mip3.w, pl.mip3.h, pl.la.lb != nullptr,
                  pl.kernel == kCompPair && pl.la.shaded != nullptr);
    out += line;
    if (pl.fold) out += "kernel\thistogram_fold\t-\t1x1x1\t256x1x1\n";
    if (pl.histogram_pass) out += "pass\tgenerate_luminance_histogram\n";
    return copy_text(out, buf, cap);
}
