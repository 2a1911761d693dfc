// ssr.hip — ScreenSpaceReflectionTask (screen_space_reflection.inl:26-70, fragment shader :88-183) for gfx950.
//
// The reference registers the task between SSAOBlur and CloudRendering (renderer.cpp:1081-1092) and pays for it every
// frame, although Composition's read of its image is commented out (composition.inl:213-216, quirk Q12). Here it is an
// opt-in pass (soc_screen_space_reflection, soc_renderer_add_screen_space_reflection): the default graph does not run it.
//
// Per pixel: a pixel whose metallic value is below 0.01 copies its albedo; every other pixel reflects its view ray about
// the view-space normal and marches it through the depth image: a first loop with a growing step (x 1.05 per iteration)
// until the ray passes behind the depth image, then a binary search with a halving step, 50 iterations over both. A probe
// within 0.05 of the depth image is a hit (the albedo at the probe's screen position); a ray that finds nothing writes
// (0, 0, 0, 1): the shader's `out_ssr == vec4(0)` fallback (:180-182) cannot fire because alpha is already 1 (quirk Q13).
//
// Arithmetic: the file is compiled without implicit contraction and uses no fma. The chain that decides a branch
// (projection, divide, tap coordinates, unprojection, delta) is the operation order of tests/ssr_oracle.py, with IEEE
// division and square root, so a branch can differ from the fp32 oracle's only through a different rounding of one of
// these operations, never through a different formula.
//
// Shape: one pixel per lane, each wave an 8 x 8 pixel tile (a 16 x 16 tile per 256-lane workgroup), so the depth taps
// of a wave's rays stay close. The two loops are one loop with a per-lane phase: a lane in its binary search iterates
// beside its neighbours still in the first loop, and the wave leaves the loop when its last lane has ended.
#include "soc_internal.hpp"

namespace soc {
namespace {

constexpr int kSsrIterations = 50;     // iterationCount, :98
constexpr int kSsrStepsMiss = 50, kSsrStepsCopy = 255;

struct SsrParams {
    Mat4 proj, inv_proj, view;
};

// (x > 0) - (x < 0): NaN gives 0 (GLSL sign() of a NaN is undefined)
__device__ __forceinline__ float ssr_sign(float x) { return (float)(x > 0.0f) - (float)(x < 0.0f); }

template <bool STEPS>
__global__ __launch_bounds__(kWorkgroup) void ssr_kernel(DImg depth, DImg normal, DImg albedo, DImg mr, DImg target, DImg steps,
                                                  SsrParams p) {
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int x = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    const int y = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (x >= target.w || y >= target.h) return;

    // :169-174 (pixel-centre taps of same-size images are texel loads)
    const f4 rm = fetch_h4(mr, x, y);
    if (rm.y < 0.01f) {
        f4 a = fetch_h4(albedo, x, y);
        a.w = 1.0f;
        row_ptr_w<uint2>(target, y)[x] = pack_h4(a);
        if (STEPS) row_ptr_w<uint8_t>(steps, y)[x] = (uint8_t)kSsrStepsCopy;
        return;
    }

    const BufImg dbuf = buf_img(depth);
    // get_view_position_from_depth, :88-95
    const float u = centre_uv(x, target.w), v = centre_uv(y, target.h);
    const f4 vp = mul(p.inv_proj, f4{u * 2.0f - 1.0f, v * 2.0f - 1.0f, fetch_f32(depth, x, y), 1.0f});
    const f3 pos = f3{vp.x / vp.w, vp.y / vp.w, vp.z / vp.w};
    // :177-178
    const f4 nt = fetch_h4(normal, x, y);
    const f3 n = normalize3(mul3of4(p.view, f3{nt.x, nt.y, nt.z}));
    const float k = 2.0f * dot3(n, pos);
    const f3 refl = normalize3(pos - n * k);

    // ssr(), :119-162
    f3 step = refl * 0.5f;
    f3 mpos = pos + step;
    float sgn = 0.0f;
    bool binary = false;     // in the second loop (:147-159)
    int i = 0, found = kSsrStepsMiss;
    float sx = 0.0f, sy = 0.0f;
    for (;;) {
        if (binary) {        // :149-150
            step = step * 0.5f;
            mpos = mpos - step * sgn;
        }
        // generateProjectedPosition, :113-117
        const f4 c = mul(p.proj, f4{mpos.x, mpos.y, mpos.z, 1.0f});
        sx = (c.x / c.w) * 0.5f + 0.5f;
        sy = (c.y / c.w) * 0.5f + 0.5f;
        const float dd = sample_f32(dbuf, sx, sy);
        const f4 e = mul(p.inv_proj, f4{sx * 2.0f - 1.0f, sy * 2.0f - 1.0f, dd, 1.0f});
        const float delta = fabsf(mpos.z) - fabsf(e.z / e.w);
        if (fabsf(delta) < 0.05f) {      // :131, :156
            found = i;
            break;
        }
        sgn = ssr_sign(delta);
        if (!binary && delta > 0.0f) {   // :135-137: leaves the first loop without incrementing i
            binary = true;
            continue;
        }
        if (!binary) {                   // :139-144
            step = step * (1.0f - 0.5f * fmaxf(sgn, 0.0f));
            mpos = mpos + step * (-sgn);
            step = step * 1.05f;
        }
        if (++i >= kSsrIterations) break;   // a first loop that ran out leaves no second loop
    }

    f4 out = f4{0.0f, 0.0f, 0.0f, 1.0f};
    if (found != kSsrStepsMiss) {
        out = sample_h4(albedo, sx, sy);
        out.w = 1.0f;
    }
    row_ptr_w<uint2>(target, y)[x] = pack_h4(out);
    if (STEPS) row_ptr_w<uint8_t>(steps, y)[x] = (uint8_t)found;
}

}  // namespace
}  // namespace soc

using namespace soc;

extern "C" int soc_screen_space_reflection(const soc_globals* g, soc_img depth, soc_img normal, soc_img albedo,
                                           soc_img metallic_roughness, soc_img target, soc_img steps, soc_stream stream) {
    const char* fn = "soc_screen_space_reflection";
    if (!g) return set_error(SOC_E_INVALID_ARG, "%s: null globals", fn);
    int rc = check_img(depth, SOC_FMT_D32F, fn, "depth");
    if (!rc) rc = check_img(normal, SOC_FMT_RGBA16F, fn, "normal");
    if (!rc) rc = check_img(albedo, SOC_FMT_RGBA16F, fn, "albedo");
    if (!rc) rc = check_img(metallic_roughness, SOC_FMT_RGBA16F, fn, "metallic_roughness");
    if (!rc) rc = check_img(target, SOC_FMT_RGBA16F, fn, "target");
    if (!rc && steps.data) rc = check_img(steps, SOC_FMT_R8_UNORM, fn, "steps");
    if (rc) return rc;
    if (target.width > 8192 || target.height > 8192)
        return set_error(SOC_E_INVALID_ARG, "%s: extent %dx%d above 8192", fn, target.width, target.height);
    const soc_img* same[] = {&depth, &normal, &albedo, &metallic_roughness, &steps};
    const char* names[] = {"depth", "normal", "albedo", "metallic_roughness", "steps"};
    for (int i = 0; i < 5; ++i) {
        if (!same[i]->data) continue;   // steps absent
        if (same[i]->width != target.width || same[i]->height != target.height)
            return set_error(SOC_E_SHAPE, "%s: %s is %dx%d, the target %dx%d", fn, names[i], same[i]->width, same[i]->height,
                             target.width, target.height);
    }
    // the depth taps address the image with 32-bit byte offsets (soc_device.hpp BufImg)
    if (!buffer_range_ok(depth)) return set_error(SOC_E_SHAPE, "%s: depth image exceeds the 2 GiB buffer-offset range", fn);
    SsrParams p;
    p.proj = mat4(g->camera_projection_matrix);
    p.inv_proj = mat4(g->camera_inverse_projection_matrix);
    p.view = mat4(g->camera_view_matrix);
    const dim3 blk(kWorkgroup), grd(ceil_div(target.width, 16), ceil_div(target.height, 16));
    if (steps.data)
        launch("ssr_kernel", kWorkgroup, ssr_kernel<true>, grd, blk, 0, hs(stream), dimg(depth), dimg(normal), dimg(albedo),
               dimg(metallic_roughness), dimg(target), dimg(steps), p);
    else
        launch("ssr_kernel", kWorkgroup, ssr_kernel<false>, grd, blk, 0, hs(stream), dimg(depth), dimg(normal), dimg(albedo),
               dimg(metallic_roughness), dimg(target), dimg(steps), p);
    return check_launch("screen_space_reflection");
}
