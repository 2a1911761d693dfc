// raster_sampler.hpp — the G-buffer resolve's texture sampler (included by raster.hip only): RGBA8 / sRGB texel decode,
// the bilinear REPEAT sample of one level, and the trilinear + anisotropic sample of a mip-chained texture in three forms
// that differ only in where a tap's texels come from: one image (sample_texture_mip), two images of one extent on shared
// axes (_mip2), or those two's interleaved paired texels (_mip2p). The footprint (mip_footprint) and the tap loop
// (mip_filter) are written once, so the three give the same bits by construction.
#pragma once

#include "luminance.hpp"
#include "soc_internal.hpp"

namespace soc {
namespace {

__device__ __forceinline__ float srgb_to_linear(float c) {
    return c <= 0.04045f ? c / 12.92f : powf((c + 0.055f) / 1.055f, 2.4f);
}

// lut: srgb_to_linear(unorm8(i)) for i in 0..255 (LDS, filled per workgroup)
__device__ __forceinline__ f4 decode_rgba8(uint32_t u, bool srgb, const float* lut) {
    const float a = unorm8(u >> 24);
    if (!srgb) return f4{unorm8(u & 255u), unorm8((u >> 8) & 255u), unorm8((u >> 16) & 255u), a};
    return f4{lut[u & 255u], lut[(u >> 8) & 255u], lut[(u >> 16) & 255u], a};
}

typedef uint32_t u2a4 __attribute__((ext_vector_type(2))) __attribute__((aligned(4)));
// The two texels (x0, y), (x1, y) of a bilinear tap's row: one 8-byte load when x1 = x0 + 1 (every tap that does
// not wrap around the REPEAT edge), else two. The same texels either way.
__device__ __forceinline__ void texel_row_pair(const DImg& im, int x0, int x1, int y, uint32_t& a, uint32_t& b) {
    const uint32_t* row = row_ptr<uint32_t>(im, y);
    if (x1 == x0 + 1) {
        const u2a4 t = *reinterpret_cast<const u2a4*>(row + x0);
        a = t.x;
        b = t.y;
    } else {
        a = row[x0];
        b = row[x1];
    }
}

// REPEAT axis of extent n: the power-of-two mask when n is one (every texture of the reference's assets),
// else the general modulo; same taps and weight either way.
__device__ __forceinline__ Axis axis_repeat_level(float u, int n) {
    return (n & (n - 1)) ? axis_repeat_any(u, n) : axis_repeat_pow2(u, n, n - 1);
}

// Bilinear REPEAT sample of one level (its image view already resolved) of a packed mip chain, from the
// level's two axes (computed once when two textures of the same extent share them).
#ifndef SOC_GB_FAST_FILTER
#define SOC_GB_FAST_FILTER 1
#endif
#if SOC_GB_FAST_FILTER
typedef unsigned short gb_u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t gb_udot2(uint32_t a, uint32_t b) {
    return __builtin_amdgcn_udot2(__builtin_bit_cast(gb_u16x2, a), __builtin_bit_cast(gb_u16x2, b), 0u, false);
}
// Bilinear of the RGBA8 texels a b (top row) / c d with the contract's 8-bit weights (w = k / 256, exact).
// UNORM: the exact integer bilinear per channel (v_dot2_u32_u16: a_k (256 - kx) + b_k kx per row, then across the rows;
// at most 255 * 65536 < 2^24, exact in fp32), one conversion and one scale per channel. sRGB: the LUT-decoded channels,
// each lerp fma(w, q - p, p). Against the oracle's unorm8-then-lerp chain this changes fp32 roundings only (the
// G-buffer's RGBA16F tolerance; the GPU LUT already differs from the oracle's powf by an ulp).
__device__ __forceinline__ f4 bilerp_rgba8(uint32_t ua, uint32_t ub, uint32_t uc, uint32_t ud, float wx, float wy, bool srgb,
                                           const float* lut) {
    if (!srgb) {
        const uint32_t kx = (uint32_t)(wx * 256.0f), ky = (uint32_t)(wy * 256.0f);
        const uint32_t wxp = (256u - kx) | (kx << 16), wyp = (256u - ky) | (ky << 16);
        constexpr float kScale = 1.0f / (255.0f * 65536.0f);
        auto ch = [&](uint32_t k) {   // channel k: bytes k of (a, b) and of (c, d) as 16-bit pairs
            const uint32_t sel = k | 0x0c00u | ((4u + k) << 16) | 0x0c000000u;
            const uint32_t top = gb_udot2(__builtin_amdgcn_perm(ub, ua, sel), wxp);
            const uint32_t bot = gb_udot2(__builtin_amdgcn_perm(ud, uc, sel), wxp);
            return (float)gb_udot2(top | (bot << 16), wyp) * kScale;
        };
        return f4{ch(0), ch(1), ch(2), ch(3)};
    }
    auto ch = [&](float a, float b, float c, float d) {
        const float top = __builtin_fmaf(wx, b - a, a), bot = __builtin_fmaf(wx, d - c, c);
        return __builtin_fmaf(wy, bot - top, top);
    };
    return f4{ch(lut[ua & 255u], lut[ub & 255u], lut[uc & 255u], lut[ud & 255u]),
              ch(lut[(ua >> 8) & 255u], lut[(ub >> 8) & 255u], lut[(uc >> 8) & 255u], lut[(ud >> 8) & 255u]),
              ch(lut[(ua >> 16) & 255u], lut[(ub >> 16) & 255u], lut[(uc >> 16) & 255u], lut[(ud >> 16) & 255u]),
              ch(unorm8(ua >> 24), unorm8(ub >> 24), unorm8(uc >> 24), unorm8(ud >> 24))};
}
// trilinear blend of two levels' samples: fma(f, s1 - s0, s0) per channel
__device__ __forceinline__ f4 lerp_levels(f4 s0, f4 s1, float f) {
    return f4{__builtin_fmaf(f, s1.x - s0.x, s0.x), __builtin_fmaf(f, s1.y - s0.y, s0.y), __builtin_fmaf(f, s1.z - s0.z, s0.z),
              __builtin_fmaf(f, s1.w - s0.w, s0.w)};
}
#else
__device__ __forceinline__ f4 lerp_levels(f4 s0, f4 s1, float f) {
    return f4{lerp_w(s0.x, s1.x, f), lerp_w(s0.y, s1.y, f), lerp_w(s0.z, s1.z, f), lerp_w(s0.w, s1.w, f)};
}
#endif

__device__ __forceinline__ f4 sample_level_ax(const DImg& im, const Axis& ax, const Axis& ay, bool srgb, const float* lut) {
    uint32_t ua, ub, uc, ud;
    texel_row_pair(im, ax.i0, ax.i1, ay.i0, ua, ub);
    texel_row_pair(im, ax.i0, ax.i1, ay.i1, uc, ud);
#if SOC_GB_FAST_FILTER
    return bilerp_rgba8(ua, ub, uc, ud, ax.w, ay.w, srgb, lut);
#else
    const f4 a = decode_rgba8(ua, srgb, lut), b = decode_rgba8(ub, srgb, lut);
    const f4 c = decode_rgba8(uc, srgb, lut), d = decode_rgba8(ud, srgb, lut);
    return bilerp4(a, b, c, d, ax.w, ay.w);
#endif
}
__device__ __forceinline__ f4 sample_texture(const soc_img& tex, float u, float v, const float* lut) {
    if (!tex.data) return f4{1.0f, 1.0f, 1.0f, 1.0f};
    const DImg im{static_cast<char*>(tex.data), tex.width, tex.height, tex.pitch_bytes};
    const bool srgb = tex.format == SOC_FMT_RGBA8_SRGB;
    return sample_level_ax(im, axis_repeat_level(u, tex.width), axis_repeat_level(v, tex.height), srgb, lut);
}
__device__ __forceinline__ DImg level_view(const soc_img& tex, int k) {
    int wk, hk;
    const size_t off = mip_offset(tex.width, tex.height, tex.pitch_bytes, k, wk, hk);
    return DImg{static_cast<char*>(tex.data) + off, wk, hk, k ? 4 * wk : tex.pitch_bytes};
}

// Fine uv derivatives of the pixel's quad.
struct UVGrad { float dudx, dvdx, dudy, dvdy; };

// What the pixel's uv footprint decides for a texture of one extent, whatever its texels: the anisotropic tap count n
// (along the major axis, <= max_aniso), the lod in 1/256 steps lq, clamped to [0, (L - 1) 256], its level pair l0, l1
// with the trilinear weight f = (lq & 255) / 256, and which screen direction is the major axis.
struct MipFootprint {
    int n, lq, l0, l1;
    float f;
    bool xmajor;
};
__device__ __forceinline__ MipFootprint mip_footprint(int width, int height, const UVGrad& gr, float max_aniso) {
#pragma clang fp contract(off)
    MipFootprint fp;
    const int L = mip_levels(width, height);
    const float W = (float)width, H = (float)height;
    const float ax = gr.dudx * W, ay = gr.dvdx * H, bx = gr.dudy * W, by = gr.dvdy * H;
    const float px = sqrtf(ax * ax + ay * ay), py = sqrtf(bx * bx + by * by);
    const float pmax = fmaxf(px, py), pmin = fminf(px, py);
    fp.n = 1;
    if (max_aniso > 1.0f && pmax > 0.0f && pmax <= 3.4e38f) {
        const float cap = floorf(max_aniso);
        fp.n = (int)(pmin > 0.0f ? fminf(ceilf(pmax / pmin), cap) : cap);
    }
    fp.lq = 0;
    const float rho = pmax / (float)fp.n;
    if (rho > 0.0f && rho <= 3.4e38f) {
        const float lam = fminf(fmaxf(det_log2(rho), -64.0f), 64.0f);
        fp.lq = min(max((int)floorf(lam * 256.0f + 0.5f), 0), (L - 1) * 256);
    }
    fp.l0 = fp.lq >> 8;
    fp.l1 = min(fp.l0 + 1, L - 1);
    fp.f = (float)(fp.lq & 255) * (1.0f / 256.0f);
    fp.xmajor = px >= py;
    return fp;
}

// Two textures' samples at one tap (sample_texture_mip2 / _mip2p): every operation is f4's, per member, a's first.
struct f4x2 { f4 a, b; };
__device__ __forceinline__ f4x2 lerp_levels(const f4x2& s0, const f4x2& s1, float f) {
    return f4x2{lerp_levels(s0.a, s1.a, f), lerp_levels(s0.b, s1.b, f)};
}
__device__ __forceinline__ f4 tap_sum(f4 s, f4 t) {
#pragma clang fp contract(off)
    return f4{s.x + t.x, s.y + t.y, s.z + t.z, s.w + t.w};
}
__device__ __forceinline__ f4x2 tap_sum(const f4x2& s, const f4x2& t) { return f4x2{tap_sum(s.a, t.a), tap_sum(s.b, t.b)}; }
__device__ __forceinline__ f4 tap_mean(f4 s, float fn) {
#pragma clang fp contract(off)
    return f4{s.x / fn, s.y / fn, s.z / fn, s.w / fn};
}
__device__ __forceinline__ f4x2 tap_mean(const f4x2& s, float fn) { return f4x2{tap_mean(s.a, fn), tap_mean(s.b, fn)}; }

// The tap loop of the trilinear + anisotropic sample: n taps spread along the major axis of the footprint, each the
// level pair's samples blended by f (level l0 alone when f = 0), summed in tap order and divided by n. V is f4 or f4x2;
// level(k, su, sv) samples level l0 (k = 0) or l1 (k = 1) at the tap's uv.
template <typename V, typename Level>
__device__ __forceinline__ V mip_filter(const MipFootprint& fp, const UVGrad& gr, float u, float v, Level&& level) {
#pragma clang fp contract(off)
    const int n = fp.n;
    const float du = fp.xmajor ? gr.dudx : gr.dudy, dv = fp.xmajor ? gr.dvdx : gr.dvdy;
    V acc{};
    for (int i = 1; i <= n; ++i) {
        float su = u, sv = v;
        if (n > 1) {
            const float t = (float)i / (float)(n + 1) - 0.5f;
            su = u + t * du;
            sv = v + t * dv;
        }
        V s = level(0, su, sv);
        if (fp.lq & 255) s = lerp_levels(s, level(1, su, sv), fp.f);
        acc = tap_sum(acc, s);
    }
    if (n == 1) return acc;
    return tap_mean(acc, (float)n);
}

// Trilinear + anisotropic REPEAT sample of a mip-chained texture (soc_rt.h SOC_MATERIAL_MIPMAPPED).
__device__ __forceinline__ f4 sample_texture_mip(const soc_img& tex, float u, float v, const UVGrad& gr, float max_aniso, const float* lut) {
    if (!tex.data) return f4{1.0f, 1.0f, 1.0f, 1.0f};
    const bool srgb = tex.format == SOC_FMT_RGBA8_SRGB;
    const MipFootprint fp = mip_footprint(tex.width, tex.height, gr, max_aniso);
    const DImg im0 = level_view(tex, fp.l0), im1 = level_view(tex, fp.l1);
    return mip_filter<f4>(fp, gr, u, v, [&](int k, float su, float sv) {
        const DImg& im = k ? im1 : im0;
        return sample_level_ax(im, axis_repeat_level(su, im.w), axis_repeat_level(sv, im.h), srgb, lut);
    });
}

// sample_texture_mip of two textures of the same extent at the same uv (the material's normal image and
// albedo): the footprint, tap count, lod and every tap's level axes depend only on the extent, so they are
// computed once; each texture's taps, lerps and sums are sample_texture_mip's, in its order (same bits).
// Precondition: both have data and ta.width == tb.width, ta.height == tb.height.
__device__ __forceinline__ void sample_texture_mip2(const soc_img& ta, const soc_img& tb, float u, float v, const UVGrad& gr,
                                    float max_aniso, const float* lut, f4& ra, f4& rb) {
    const bool sa = ta.format == SOC_FMT_RGBA8_SRGB, sb = tb.format == SOC_FMT_RGBA8_SRGB;
    const MipFootprint fp = mip_footprint(ta.width, ta.height, gr, max_aniso);
    const DImg a0 = level_view(ta, fp.l0), a1 = level_view(ta, fp.l1), b0 = level_view(tb, fp.l0), b1 = level_view(tb, fp.l1);
    const f4x2 r = mip_filter<f4x2>(fp, gr, u, v, [&](int k, float su, float sv) {
        const DImg &a = k ? a1 : a0, &b = k ? b1 : b0;
        const Axis x = axis_repeat_level(su, a.w), y = axis_repeat_level(sv, a.h);
        return f4x2{sample_level_ax(a, x, y, sa, lut), sample_level_ax(b, x, y, sb, lut)};
    });
    ra = r.a;
    rb = r.b;
}

// sample_texture_mip2 from the material's paired texels (soc_pair_textures: albedo and normal texel interleaved, 8 B):
// each tap row of both textures is one 16-B load (two 8-B loads at the REPEAT seam) instead of one 8-B load per
// texture. The same texels reach the same filter arithmetic: the same bits as sample_texture_mip2 (GPU test).
__device__ __forceinline__ DImg paired_level(const void* paired, int W, int H, int k) {
    int wk, hk;
    const size_t off = mip_offset(W, H, 8 * W, k, wk, hk, 8);
    return DImg{static_cast<char*>(const_cast<void*>(paired)) + off, wk, hk, 8 * wk};
}
typedef uint32_t u4a8g __attribute__((ext_vector_type(4))) __attribute__((aligned(8)));
__device__ __forceinline__ void paired_row(const DImg& im, int x0, int x1, int y, uint32_t& a0, uint32_t& n0, uint32_t& a1,
                                           uint32_t& n1) {
    const uint2* row = row_ptr<uint2>(im, y);
    if (x1 == x0 + 1) {
        const u4a8g t = *reinterpret_cast<const u4a8g*>(row + x0);
        a0 = t.x; n0 = t.y; a1 = t.z; n1 = t.w;
    } else {
        const uint2 p = row[x0], q = row[x1];
        a0 = p.x; n0 = p.y; a1 = q.x; n1 = q.y;
    }
}
__device__ __forceinline__ void sample_paired_level(const DImg& im, const Axis& ax, const Axis& ay, bool sn, bool sa,
                                                    const float* lut, f4& rn, f4& ra) {
    uint32_t a0, n0, a1, n1, a2, n2, a3, n3;
    paired_row(im, ax.i0, ax.i1, ay.i0, a0, n0, a1, n1);
    paired_row(im, ax.i0, ax.i1, ay.i1, a2, n2, a3, n3);
#if SOC_GB_FAST_FILTER
    rn = bilerp_rgba8(n0, n1, n2, n3, ax.w, ay.w, sn, lut);
    ra = bilerp_rgba8(a0, a1, a2, a3, ax.w, ay.w, sa, lut);
#else
    rn = bilerp4(decode_rgba8(n0, sn, lut), decode_rgba8(n1, sn, lut), decode_rgba8(n2, sn, lut), decode_rgba8(n3, sn, lut), ax.w, ay.w);
    ra = bilerp4(decode_rgba8(a0, sa, lut), decode_rgba8(a1, sa, lut), decode_rgba8(a2, sa, lut), decode_rgba8(a3, sa, lut), ax.w, ay.w);
#endif
}
// ta: the normal image, tb: the albedo (their extent and formats); results as sample_texture_mip2's (ra: normal, rb: albedo)
__device__ __forceinline__ void sample_texture_mip2p(const soc_img& ta, const soc_img& tb, const void* paired, float u, float v,
                                                     const UVGrad& gr, float max_aniso, const float* lut, f4& ra, f4& rb) {
    const bool sa = ta.format == SOC_FMT_RGBA8_SRGB, sb = tb.format == SOC_FMT_RGBA8_SRGB;
    const MipFootprint fp = mip_footprint(ta.width, ta.height, gr, max_aniso);
    const DImg p0 = paired_level(paired, ta.width, ta.height, fp.l0), p1 = paired_level(paired, ta.width, ta.height, fp.l1);
    const f4x2 r = mip_filter<f4x2>(fp, gr, u, v, [&](int k, float su, float sv) {
        const DImg& p = k ? p1 : p0;
        f4x2 s;
        sample_paired_level(p, axis_repeat_level(su, p.w), axis_repeat_level(sv, p.h), sa, sb, lut, s.a, s.b);
        return s;
    });
    ra = r.a;
    rb = r.b;
}

}  // namespace
}  // namespace soc
