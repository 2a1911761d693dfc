// dof.hip — the reference's depth-of-field task chain (depth_of_field.inl) for gfx950: BlitImageToImage (:16-48),
// MipMapping - i (:55-88, registered per level in renderer.cpp:1127-1144) and DepthOfField (:104-155, fragment shader
// :176-199). The reference has the three add_task calls commented out (renderer.cpp:1119-1153); here they are an opt-in
// pair of passes (soc_depth_of_field_mips, soc_depth_of_field, soc_renderer_add_depth_of_field): the default graph does
// not run them.
//
// The chain (tasks 1 and 2): depth_of_field_image is RGBA16F with floor(log2(max(W, H))) + 1 levels (renderer.cpp:346,
// 463-468). Level 0 is a same-size LINEAR blit of the colour image, i.e. its texels; level k is a LINEAR blit of level
// k - 1: texture.hip's arithmetic (blit_axis: clamp to edge, 8-bit weights; bilerp4 on the f16 texels widened to f32,
// no contraction) with all four channels rounded to f16 nearest-even. The packed layout is soc_generate_mips's at
// 8 B per texel. Two forms that give the same bits (tuning knob SOC_DOF_CHAIN_FUSED, default 1):
//   per-level  one copy launch and one blit launch per level (the measured baseline),
//   fused      a head kernel that reads each 2 x 2 colour footprint once and writes its four level-0 texels and its
//              level-1 texel (even extents: blit_axis is then exactly taps (2x, 2x + 1) with weight 1/2; odd extents keep
//              the copy and the general blit), per-level launches for the middle levels, and one single-workgroup tail
//              launch for every level of at most kDofTailTexels texels (a workgroup-wide barrier between levels).
//
// The pass (task 3): one pixel per lane, 8 x 8-pixel wave footprints as in ssr.hip. A pixel with depth < 1 is the mean
// of four textureGrad taps of the chain at uv +- (1/W, 0), uv +- (0, 1/H) with both gradients (c, c), c = coc / max_coc
// (:180-189), through depth_of_field_sampler (renderer.cpp:472-488: trilinear, REPEAT, anisotropy 16, max_lod = L); its
// alpha is 1. Any other pixel (NaN depth included) is the chain's level-0 texel. The gradients are equal, so the
// footprint is a circle: one tap position per textureGrad, the anisotropy never engages; the LOD follows
// sample_texture_mip's conventions (raster.hip) in 1/256 steps, clamped to level L - 1 (max_lod is past the last level).
// All four taps share the pixel's two levels and blend factor; the second level is skipped when the fraction is 0.
// Arithmetic: f32, no contraction, IEEE division and square root, in the operation order of tests/dof_oracle.py.
#include "luminance.hpp"
#include "soc_internal.hpp"

namespace soc {
namespace {

constexpr int kDofMaxLevels = 14;        // an extent of at most 8192: floor(log2(8192)) + 1
constexpr int kDofMaxExtent = 8192;
constexpr int kDofTailTexels = 4096;     // the tail launch takes every level of at most this many texels

// The chain's levels (host-built, a kernel argument): byte offset from level 0's first texel, extent, row pitch.
struct DofLevels {
    unsigned long long off[kDofMaxLevels];
    int w[kDofMaxLevels], h[kDofMaxLevels], pitch[kDofMaxLevels];
    int count;
};
struct DofLevel {
    unsigned long long off;
    int w, h, pitch;
};

DofLevels dof_levels(int W, int H, int pitch) {
    DofLevels lv{};
    lv.count = mip_levels(W, H);
    for (int k = 0; k < lv.count; ++k) {
        int wk, hk;
        lv.off[k] = mip_offset(W, H, pitch, k, wk, hk, 8);
        lv.w[k] = wk;
        lv.h[k] = hk;
        lv.pitch[k] = k ? 8 * wk : pitch;
    }
    return lv;
}

DImg level_img(char* base, const DofLevels& lv, int k) { return DImg{base + lv.off[k], lv.w[k], lv.h[k], lv.pitch[k]}; }

// One destination texel of a LINEAR blit src -> (dw x dh): mip_blit's taps and weights on RGBA16F texels.
__device__ __forceinline__ uint2 dof_blit_texel(const DImg& src, int x, int y, int dw, int dh) {
    const Axis ax = blit_axis(x, src.w, dw), ay = blit_axis(y, src.h, dh);
    const uint2* r0 = row_ptr<uint2>(src, ay.i0);
    const uint2* r1 = row_ptr<uint2>(src, ay.i1);
    return pack_h4(bilerp4(unpack_h4(r0[ax.i0]), unpack_h4(r0[ax.i1]), unpack_h4(r1[ax.i0]), unpack_h4(r1[ax.i1]), ax.w, ay.w));
}

// BlitImageToImage: level 0 <- the colour's texels.
__global__ __launch_bounds__(kWorkgroup) void dof_copy(DImg src, DImg dst) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= dst.w || y >= dst.h) return;
    row_ptr_w<uint2>(dst, y)[x] = row_ptr<uint2>(src, y)[x];
}

// MipMapping - i: one level, one lane per destination texel.
__global__ __launch_bounds__(kWorkgroup) void dof_blit(DImg src, DImg dst) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= dst.w || y >= dst.h) return;
    row_ptr_w<uint2>(dst, y)[x] = dof_blit_texel(src, x, y, dst.w, dst.h);
}

// Head of the fused form (even extents): one lane per level-1 texel reads its 2 x 2 colour footprint (one 16-B load per
// row), stores the four texels to level 0 and their blit to level 1: blit_axis(x, 2n, n) is taps (2x, 2x + 1) with
// weight 1/2 exactly ((2x + 1) 2n / 2n - 0.5 = 2x + 0.5 in f32 for n <= 8192), so this is dof_blit's arithmetic.
__global__ __launch_bounds__(kWorkgroup) void dof_head(DImg color, DImg l0, DImg l1) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= l1.w || y >= l1.h) return;
    const soc_u4a4 top = *reinterpret_cast<const soc_u4a4*>(row_ptr<uint2>(color, 2 * y) + 2 * x);
    const soc_u4a4 bot = *reinterpret_cast<const soc_u4a4*>(row_ptr<uint2>(color, 2 * y + 1) + 2 * x);
    *reinterpret_cast<soc_u4a4*>(row_ptr_w<uint2>(l0, 2 * y) + 2 * x) = top;
    *reinterpret_cast<soc_u4a4*>(row_ptr_w<uint2>(l0, 2 * y + 1) + 2 * x) = bot;
    row_ptr_w<uint2>(l1, y)[x] = pack_h4(bilerp4(unpack_h4(uint2{top.x, top.y}), unpack_h4(uint2{top.z, top.w}),
                                                 unpack_h4(uint2{bot.x, bot.y}), unpack_h4(uint2{bot.z, bot.w}), 0.5f, 0.5f));
}

// Tail of the fused form: one workgroup builds levels first .. count - 1 one after another; a level's texels are in
// memory (device-scope fence) before the barrier that lets the next level read them.
__global__ __launch_bounds__(kWorkgroup) void dof_tail(char* chain, DofLevels lv, int first) {
    for (int k = first; k < lv.count; ++k) {
        const DImg src{chain + lv.off[k - 1], lv.w[k - 1], lv.h[k - 1], lv.pitch[k - 1]};
        const DImg dst{chain + lv.off[k], lv.w[k], lv.h[k], lv.pitch[k]};
        for (int i = threadIdx.x; i < dst.w * dst.h; i += kWorkgroup) {
            const int y = i / dst.w, x = i - y * dst.w;
            row_ptr_w<uint2>(dst, y)[x] = dof_blit_texel(src, x, y, dst.w, dst.h);
        }
        __threadfence();
        __syncthreads();
    }
}

struct DofParams {
    float near_clip, far_clip, focal_length, plane_in_focus, aperture;
};

// axis_repeat_any for a coordinate within one texel of [0, 1] (the pass's taps: a pixel centre +- one level-0 texel, so
// the left tap index is in [-n, 2n) at every level): the wrap-around is one conditional add or subtract instead of two
// integer divisions. Any other coordinate takes axis_repeat_any's modulo: the same taps and weight always.
__device__ __forceinline__ Axis dof_axis(float u, int n) {
#pragma clang fp contract(off)
    float t = u * (float)n;
    t = t - 0.5f;
    t = fminf(fmaxf(t, -4194304.0f), 4194304.0f);
    const int fx = (int)floorf(t * 256.0f + 0.5f);
    const int i = fx >> 8;
    Axis a;
    a.w = (float)(fx & 255) * (1.0f / 256.0f);
    int r = i < 0 ? i + n : (i >= n ? i - n : i);
    if ((unsigned)r >= (unsigned)n) {
        r = i % n;
        if (r < 0) r += n;
    }
    a.i0 = r;
    a.i1 = r + 1 == n ? 0 : r + 1;
    return a;
}

// One bilinear REPEAT tap of a level (axis_repeat_any's taps and 8-bit weights, bilerp4): a row's texel pair is one
// 16-B load unless the tap wraps around the edge.
__device__ __forceinline__ f4 dof_tap(const char* chain, const DofLevel& l, const Axis& ax, const Axis& ay) {
    const uint2* r0 = reinterpret_cast<const uint2*>(chain + l.off + (size_t)ay.i0 * (size_t)l.pitch);
    const uint2* r1 = reinterpret_cast<const uint2*>(chain + l.off + (size_t)ay.i1 * (size_t)l.pitch);
    uint2 a, b, c, d;
    if (ax.i1 == ax.i0 + 1) {
        const soc_u4a4 p0 = *reinterpret_cast<const soc_u4a4*>(r0 + ax.i0);
        const soc_u4a4 p1 = *reinterpret_cast<const soc_u4a4*>(r1 + ax.i0);
        a = uint2{p0.x, p0.y};
        b = uint2{p0.z, p0.w};
        c = uint2{p1.x, p1.y};
        d = uint2{p1.z, p1.w};
    } else {
        a = r0[ax.i0];
        b = r0[ax.i1];
        c = r1[ax.i0];
        d = r1[ax.i1];
    }
    return bilerp4(unpack_h4(a), unpack_h4(b), unpack_h4(c), unpack_h4(d), ax.w, ay.w);
}

__global__ __launch_bounds__(kWorkgroup) void dof_kernel(DImg depth, const char* chain, DofLevels lv, DImg target, DofParams p) {
#pragma clang fp contract(off)
    // the level table in LDS: a lane's two levels are data-dependent
    __shared__ DofLevel s_lv[kDofMaxLevels];
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < kDofMaxLevels; ++k)
        if (tid == k && k < lv.count) s_lv[k] = DofLevel{lv.off[k], lv.w[k], lv.h[k], lv.pitch[k]};
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    const int x = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    const int y = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (x >= target.w || y >= target.h) return;

    const float d = fetch_f32(depth, x, y);
    if (!(d < 1.0f)) {   // :196-198: a pixel-centre tap of level 0 is the texel, alpha kept
        row_ptr_w<uint2>(target, y)[x] = reinterpret_cast<const uint2*>(chain + (size_t)y * (size_t)lv.pitch[0])[x];
        return;
    }
    // :180, :187-189
    const float od = (-p.far_clip * p.near_clip) / (d * (p.far_clip - p.near_clip) - p.far_clip);
    const float den = od * (p.plane_in_focus - p.focal_length);
    const float coc = fabsf((p.aperture * (p.focal_length * (od - p.plane_in_focus))) / den);
    const float max_coc = fabsf((p.aperture * (p.focal_length * (p.far_clip - p.plane_in_focus))) / den);
    const float c = coc / max_coc;
    // textureGrad with both gradients (c, c): sample_texture_mip's lod (raster.hip), one tap position
    const float W = (float)target.w, H = (float)target.h;
    const float ax = c * W, ay = c * H;
    const float rho = sqrtf(ax * ax + ay * ay);
    const int L = lv.count;
    int lq = 0;
    if (rho > 0.0f && rho <= 3.4e38f) {
        const float lam = fminf(fmaxf(det_log2(rho), -64.0f), 64.0f);
        lq = min(max((int)floorf(lam * 256.0f + 0.5f), 0), (L - 1) * 256);
    }
    const int l0 = lq >> 8, l1 = min(l0 + 1, L - 1);
    const float f = (float)(lq & 255) * (1.0f / 256.0f);

    const float u = centre_uv(x, target.w), v = centre_uv(y, target.h);
    const float ox = 1.0f / W, oy = 1.0f / H;
    f4 t[4];
    // the taps (u +- ox, v) share their row axis, (u, v +- oy) their column axis: six axes per level
    const auto taps = [&](const DofLevel& l, f4* s) {
        const Axis xc = dof_axis(u, l.w), xp = dof_axis(u + ox, l.w), xm = dof_axis(u - ox, l.w);
        const Axis yc = dof_axis(v, l.h), yp = dof_axis(v + oy, l.h), ym = dof_axis(v - oy, l.h);
        s[0] = dof_tap(chain, l, xp, yc);
        s[1] = dof_tap(chain, l, xm, yc);
        s[2] = dof_tap(chain, l, xc, yp);
        s[3] = dof_tap(chain, l, xc, ym);
    };
    taps(s_lv[l0], t);
    if (lq & 255) {
        f4 t1[4];
        taps(s_lv[l1], t1);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f4 s1 = t1[i];
            t[i] = f4{lerp_w(t[i].x, s1.x, f), lerp_w(t[i].y, s1.y, f), lerp_w(t[i].z, s1.z, f), 1.0f};
        }
    }
    // :191-194
    const f4 out{((t[0].x * 0.25f + t[1].x * 0.25f) + t[2].x * 0.25f) + t[3].x * 0.25f,
                 ((t[0].y * 0.25f + t[1].y * 0.25f) + t[2].y * 0.25f) + t[3].y * 0.25f,
                 ((t[0].z * 0.25f + t[1].z * 0.25f) + t[2].z * 0.25f) + t[3].z * 0.25f, 1.0f};
    row_ptr_w<uint2>(target, y)[x] = pack_h4(out);
}

// [data, end) of the bytes an image view's rows cover
bool overlaps(const soc_img& im, const void* base, size_t bytes) {
    const char* a0 = static_cast<const char*>(im.data);
    const char* a1 = a0 + (size_t)im.pitch_bytes * (size_t)(im.height - 1) + (size_t)im.width * 8;
    const char* b0 = static_cast<const char*>(base);
    return a0 < b0 + bytes && b0 < a1;
}

int check_chain(const char* fn, const soc_img& chain) {
    int rc = check_img(chain, SOC_FMT_RGBA16F, fn, "chain");
    if (rc) return rc;
    if (chain.width > kDofMaxExtent || chain.height > kDofMaxExtent)
        return set_error(SOC_E_INVALID_ARG, "%s: extent %dx%d above %d", fn, chain.width, chain.height, kDofMaxExtent);
    return SOC_OK;
}

}  // namespace
}  // namespace soc

using namespace soc;

extern "C" size_t soc_depth_of_field_chain_bytes(int32_t width, int32_t height, int32_t pitch_bytes) {
    if (width <= 0 || height <= 0 || width > kDofMaxExtent || height > kDofMaxExtent || pitch_bytes < width * 8 || pitch_bytes % 8)
        return 0;
    int wk, hk;
    const int L = mip_levels(width, height);
    return mip_offset(width, height, pitch_bytes, L - 1, wk, hk, 8) + (L > 1 ? (size_t)8 * wk * hk : (size_t)pitch_bytes * height);
}

extern "C" int soc_depth_of_field_mips(soc_img color, soc_img chain, soc_stream stream) {
    const char* fn = "soc_depth_of_field_mips";
    int rc = check_img(color, SOC_FMT_RGBA16F, fn, "color");
    if (!rc) rc = check_chain(fn, chain);
    if (rc) return rc;
    if (color.width != chain.width || color.height != chain.height)
        return set_error(SOC_E_SHAPE, "%s: color is %dx%d, the chain %dx%d", fn, color.width, color.height, chain.width, chain.height);
    const int W = chain.width, H = chain.height;
    if (overlaps(color, chain.data, soc_depth_of_field_chain_bytes(W, H, chain.pitch_bytes)))
        return set_error(SOC_E_INVALID_ARG, "%s: color may not alias the chain's allocation", fn);
    const DofLevels lv = dof_levels(W, H, chain.pitch_bytes);
    char* base = static_cast<char*>(chain.data);
    hipStream_t s = hs(stream);
    const dim3 blk(64, 4);
    const auto grid = [](int w, int h) { return dim3(ceil_div(w, 64), ceil_div(h, 4)); };
    const auto blit = [&](int k) {
        launch("dof_blit", kWorkgroup, dof_blit, grid(lv.w[k], lv.h[k]), blk, 0, s, level_img(base, lv, k - 1), level_img(base, lv, k));
    };
    int k = 1;
    const bool fused = tuning_knob("SOC_DOF_CHAIN_FUSED", 1) != 0;
    if (fused && lv.count > 1 && W % 2 == 0 && H % 2 == 0) {
        launch("dof_head", kWorkgroup, dof_head, grid(lv.w[1], lv.h[1]), blk, 0, s, dimg(color), level_img(base, lv, 0),
               level_img(base, lv, 1));
        k = 2;
    } else {
        launch("dof_copy", kWorkgroup, dof_copy, grid(W, H), blk, 0, s, dimg(color), level_img(base, lv, 0));
    }
    int tail = lv.count;   // first level of the tail launch
    if (fused)
        while (tail > k && lv.w[tail - 1] * lv.h[tail - 1] <= kDofTailTexels) --tail;
    for (; k < tail; ++k) blit(k);
    if (tail < lv.count) launch("dof_tail", kWorkgroup, dof_tail, dim3(1), dim3(kWorkgroup), 0, s, base, lv, tail);
    return check_launch("depth_of_field_mips");
}

extern "C" int soc_depth_of_field(const soc_globals* g, soc_img depth, soc_img chain, soc_img target, soc_stream stream) {
    const char* fn = "soc_depth_of_field";
    if (!g) return set_error(SOC_E_INVALID_ARG, "%s: null globals", fn);
    int rc = check_img(depth, SOC_FMT_D32F, fn, "depth");
    if (!rc) rc = check_chain(fn, chain);
    if (!rc) rc = check_img(target, SOC_FMT_RGBA16F, fn, "target");
    if (rc) return rc;
    if (depth.width != target.width || depth.height != target.height)
        return set_error(SOC_E_SHAPE, "%s: depth is %dx%d, the target %dx%d", fn, depth.width, depth.height, target.width, target.height);
    if (chain.width != target.width || chain.height != target.height)
        return set_error(SOC_E_SHAPE, "%s: chain is %dx%d, the target %dx%d", fn, chain.width, chain.height, target.width, target.height);
    if (overlaps(target, chain.data, soc_depth_of_field_chain_bytes(chain.width, chain.height, chain.pitch_bytes)))
        return set_error(SOC_E_INVALID_ARG, "%s: target may not alias the chain's allocation", fn);
    const DofLevels lv = dof_levels(chain.width, chain.height, chain.pitch_bytes);
    const DofParams p{g->camera_near_clip, g->camera_far_clip, g->focal_length, g->plane_in_focus, g->aperture};
    const dim3 blk(kWorkgroup), grd(ceil_div(target.width, 16), ceil_div(target.height, 16));
    launch("dof_kernel", kWorkgroup, dof_kernel, grd, blk, 0, hs(stream), dimg(depth), static_cast<const char*>(chain.data), lv,
           dimg(target), p);
    return check_launch("depth_of_field");
}
