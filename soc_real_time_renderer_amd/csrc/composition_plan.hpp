// composition_plan.hpp — what the planner of a Composition call (composition_plan.cpp, host only, no HIP call) and its
// issuer (composition.hip) share: the call record the entry points fill, the kernel-argument structs, the kernel form as
// data, and the plan itself.
#pragma once

#include "luminance.hpp"
#include "soc_internal.hpp"

namespace soc {

struct CompParams {
    Mat4 inv_proj, inv_view, sun_pv;
    Mat4 sun_clip;        // sun_pv * inv_view * inv_proj: NDC (x, y, depth, 1) -> sun clip space
    float sun_dir[3], ambient[3], cam[3];
    float ef, df, emissive_strength, ao_strength;
    uint32_t npl, nsl;
    int swz;   // XCD-aware tile order (fast path)
    uint32_t* bins;        // fused histogram: 8 x 256 scratch copies (composition_pair<true>)
    float lmin, lrange;    // log_min_luminance, log_max - log_min
    BinFast bf;            // lum_bin_fast parameters
    const soc_globals* __restrict__ dg;  // device globals (lights), may be null when npl == nsl == 0
    int sky_external;      // 1: sky pixels (depth == 1) are written and binned by sky_compose_pair (second lane)
    float rw, rh;          // recip_rn(target extent) for the pixel-centre uv (div_rn)
    int bloom_zero_skip;   // SOC_BLOOM_ZERO_SKIP: the in-kernel bloom skips its sums on all-zero mip1 tiles (BL)
    int bloom_sparse;      // SOC_BLOOM_SPARSE: the workgroup's cell is tested against mip3 (zero_cells, bloom_w.hpp)
};
// the bounded lights' part of the parameter block (LB != 0)
struct LightArgs {
    const LightBoundsDev* lb;
    uint32_t* shaded;
};
struct CompParamsBounded : CompParams {
    LightArgs la;
};
// the cascaded sun shadows' parameter block (CS; composition.hip describes the fields where it uses them)
struct Mat4d { double m[16]; };
struct CompParamsCascaded : CompParams {
    Mat4d inv_proj_d, inv_view_d;          // the globals' fp32 entries, widened
    Mat4d pv[SOC_MAX_SUN_CASCADES];
    double rw_d, rh_d;                     // 1 / target width, 1 / target height
    float split[SOC_MAX_SUN_CASCADES - 1];
    float ef[SOC_MAX_SUN_CASCADES];
    int count, S;
};

constexpr int kLbBounded = 1, kLbCull = 2, kLbCount = 4;   // the bits of a form's lb (light_sum, composition.hip)
constexpr int kGenericBlockX = 64, kGenericBlockY = 4;    // the generic kernels' block

// One Composition call, as its entry point received it. The planner reads the host records (g, bounds, cascades and the
// two bloom mips' descriptions) and takes the address of ae's buckets; no device memory is touched before the kernels run.
struct CompositionCall {
    const soc_globals* g;
    const soc_globals* d_globals;   // device globals (the lights)
    soc_img target, albedo, emissive, normal, depth, ssao, shadow, clouds;
    // the *_luminance_histogram calls: the stored colour is binned into ae->histogram_buckets through `scratch`
    // (8 partial histograms); fold = false leaves the partials to a histogram_fold_launch of the caller's
    bool histogram;
    soc_auto_exposure* ae;
    uint32_t* scratch;
    bool fold;
    bool sky_external;             // the sky pixels are sky_compose_launch's (the render graph's second lane)
    const soc_img* bloom_mip1;     // the render graph under SOC_RENDERER_BLOOM_IN_COMPOSITION: the bloom's last stage in the kernel
    const soc_img* bloom_mip3;     // the render graph under SOC_BLOOM_SPARSE: cells proven zero from the chain's mip3
    const LightBoundsCall* bounds; // bounded lights (null: the unbounded kernels)
    const soc_sun_cascades* cascades;
    bool cascaded;                 // a cascaded entry point (a null record is then its error)
};

// composition_pair<HIST, LIGHTS, NT, BL, SP, LB, CS>'s arguments as data: the issuer's tables are indexed by them
struct PairForm {
    bool hist, lights;
    int nt;
    bool bl, sp;
    int lb;
    bool cs;
};
enum CompKernel : int { kCompPair, kCompGeneric, kCompGenericBounded, kCompGenericCascaded };

// One call's decisions. The pointers are the caller's (never dereferenced by the planner).
struct CompositionPlan {
    CompKernel kernel;
    PairForm form;                 // kCompPair only
    int grid_x, grid_y, block_x, block_y;
    DImg img[8];                   // target, albedo, emissive, normal, depth, ssao, shadow, clouds
    DImg mip1, mip3;               // null images where the form does not read them
    CompParamsCascaded p;          // the CompParams every kernel takes; its extension is filled for the cascaded kernels
    LightArgs la;                  // the bounded kernels' extension
    bool fold;                     // histogram_fold(scratch, bins) follows
    uint32_t *scratch, *bins;
    bool histogram_pass;           // not fusable: soc_generate_luminance_histogram(g, target, ae) follows
};

// Plans the call: the checks in the entry points' order (SOC_OK, or the code with the message set), the path, the kernel
// form, the grid and the parameter block. No HIP call, no image pointer dereferenced.
int plan_composition(const CompositionCall& c, CompositionPlan& out);
// The record of a call with these globals and images (target, albedo, emissive, normal, depth, ssao, shadow, clouds) and
// nothing else set.
CompositionCall composition_call(const soc_globals* g, const soc_globals* d_globals, const soc_img (&im)[8]);
// Plans the call and issues the plan on `stream` (composition.hip): what every entry point and the render graph run.
int composition(const CompositionCall& c, soc_stream stream);
// The pair path applies to the call's images (extents, even width, alignment): the one predicate behind the plan's path
// and composition_pair_applicable.
bool composition_pair_path(const CompositionCall& c);

// sky_compose_launch's plan: the CP form (a pair's clouds texels in one 8-B load), the grid and the histogram parameters
struct SkyComposePlan {
    bool pair_load;
    int grid_x, grid_y;
    DImg target, depth, clouds;
    CompParams p;
};
int plan_sky_compose(const soc_globals* g, const soc_img& target, const soc_img& depth, const soc_img& clouds,
                     uint32_t* scratch, SkyComposePlan& out);

}  // namespace soc
