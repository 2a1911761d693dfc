// composition.hip — CompositionTask (src/graphics/tasks/composition.inl:29-79, shader :110-225) as a
// gfx950 kernel.
//
// HBM-bound stream: per pixel it reads depth (4 B), albedo/emissive/normal (8 B each), one bilinear
// half-res AO tap, one bilinear 4096^2 shadow-map tap and, on sky pixels only, the clouds texel; it
// writes 8 B of RGBA16F. Fast path: two horizontally adjacent pixels per lane so every G-buffer load
// and the store are 16 B per lane, a wave covering a 16x8 pixel block (one 128-B line per image row);
// the block shape keeps the shadow-map gathers of a wave in a compact 2D patch of the map (measured:
// 89 -> 75 us at 4K against 128x1 strips). Full-res taps are plain loads (a centre sample under the
// sampling contract is the texel itself). The dead volumetric-fog block (:176-196, zeroed at :196)
// is not computed.
#include <type_traits>

#include "bloom_w.hpp"
#include "composition_plan.hpp"
#include "light_cull.hpp"

// Profiling builds only (tools/kernel_variants.py): 1 = no shadow-map tap, 2 = no AO tap, 3 = neither.
#ifndef SOC_COMP_PROFILE
#define SOC_COMP_PROFILE 0
#endif

namespace soc {
namespace {

__device__ __forceinline__ float fast_pow(float x, float y) {
    // pow(x, y) = exp2(y * log2(x)) on the native transcendental units (as the reference GPU does)
    return __builtin_amdgcn_exp2f(y * __builtin_amdgcn_logf(x));
}

// The light loops are written once over a lane type T: float (one pixel) or f2v (the lane's two pixels as packed
// f32 pairs, v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32), with the same operations in the same order, so both
// forms give the same bits per pixel. The light records are wave-uniform scalars, broadcast into both halves.
typedef float f2v __attribute__((ext_vector_type(2)));
template <class T> struct V3 { T x, y, z; };
__device__ __forceinline__ float bcv(float s, float) { return s; }
__device__ __forceinline__ f2v bcv(float s, f2v) { return f2v{s, s}; }
__device__ __forceinline__ float vfma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ f2v vfma(f2v a, f2v b, f2v c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ float vrsq(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ f2v vrsq(f2v x) { return f2v{__builtin_amdgcn_rsqf(x.x), __builtin_amdgcn_rsqf(x.y)}; }
__device__ __forceinline__ float vsqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ f2v vsqrt(f2v x) { return f2v{__builtin_amdgcn_sqrtf(x.x), __builtin_amdgcn_sqrtf(x.y)}; }
__device__ __forceinline__ float vexp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ f2v vexp2(f2v x) { return f2v{__builtin_amdgcn_exp2f(x.x), __builtin_amdgcn_exp2f(x.y)}; }
__device__ __forceinline__ float vabs(float x) { return fabsf(x); }
__device__ __forceinline__ f2v vabs(f2v x) { return f2v{fabsf(x.x), fabsf(x.y)}; }
__device__ __forceinline__ float vmax0(float x) { return fmaxf(x, 0.0f); }
__device__ __forceinline__ f2v vmax0(f2v x) { return f2v{fmaxf(x.x, 0.0f), fmaxf(x.y, 0.0f)}; }
__device__ __forceinline__ float vclamp01(float x) { return clampf(x, 0.0f, 1.0f); }
__device__ __forceinline__ f2v vclamp01(f2v x) { return f2v{clampf(x.x, 0.0f, 1.0f), clampf(x.y, 0.0f, 1.0f)}; }
__device__ __forceinline__ float vneg_pi(float x, float r) { return x < 0.0f ? 3.14159265358979f - r : r; }
__device__ __forceinline__ f2v vneg_pi(f2v x, f2v r) {
    const f2v q = f2v{3.14159265358979f, 3.14159265358979f} - r;
    return f2v{x.x < 0.0f ? q.x : r.x, x.y < 0.0f ? q.y : r.y};
}
__device__ __forceinline__ float vnan_outside1(float x, float r) { return fabsf(x) > 1.0f ? __builtin_nanf("") : r; }
__device__ __forceinline__ f2v vnan_outside1(f2v x, f2v r) {
    return f2v{fabsf(x.x) > 1.0f ? __builtin_nanf("") : r.x, fabsf(x.y) > 1.0f ? __builtin_nanf("") : r.y};
}
// a where f > 0, else b (a NaN f takes b): the select of the bounded lights, per pixel of the pair
__device__ __forceinline__ float vsel_pos(float f, float a, float b) { return f > 0.0f ? a : b; }
__device__ __forceinline__ f2v vsel_pos(f2v f, f2v a, f2v b) { return f2v{f.x > 0.0f ? a.x : b.x, f.y > 0.0f ? a.y : b.y}; }
__device__ __forceinline__ float vdiv(float a, float b) { return a / b; }
__device__ __forceinline__ f2v vdiv(f2v a, float b) { return f2v{a.x / b, a.y / b}; }
template <class T> __device__ __forceinline__ T vdot(const V3<T>& a, const V3<T>& b) {
    return vfma(a.z, b.z, vfma(a.y, b.y, a.x * b.x));
}

// acos on the native units: Abramowitz & Stegun 4.4.46, acos(a) = sqrt(1 - a) * P7(a) for a in [0, 1]
// (|error| <= 2e-8 rad), acos(x) = pi - acos(-x) below 0. Outside [-1, 1] the sqrt gives NaN, as acos does.
template <class T>
__device__ __forceinline__ T acos_fast(T x) {
    const T a = vabs(x);
    T r = bcv(-0.0012624911f, x);
    r = vfma(r, a, bcv(0.0066700901f, x));
    r = vfma(r, a, bcv(-0.0170881256f, x));
    r = vfma(r, a, bcv(0.0308918810f, x));
    r = vfma(r, a, bcv(-0.0501743046f, x));
    r = vfma(r, a, bcv(0.0889789874f, x));
    r = vfma(r, a, bcv(-0.2145988016f, x));
    r = vfma(r, a, bcv(1.5707963050f, x));
    r = r * vsqrt(bcv(1.0f, x) - a);
    return vneg_pi(x, r);
}

// exp(-acos(c)^2), the specular term of composition.inl:135-138, as one degree-10 polynomial in c (least squares on
// [-1, 1], fp32 Horner): |error| <= 1.1e-6 for c >= -0.9 and <= 2.6e-5 at c = -1, where the term itself is 5e-5 (acos is
// not analytic there; exp(-acos^2) is tiny). Ten FMAs instead of acos_fast's polynomial, square root and select plus
// the exponential: two transcendentals less per light and pixel. NaN outside [-1, 1], as acos (and acos_fast) give.
// SOC_COMP_SPEC_POLY=0 (build-time) keeps acos_fast + exp2.
#ifndef SOC_COMP_SPEC_POLY
#define SOC_COMP_SPEC_POLY 1
#endif
template <class T>
__device__ __forceinline__ T spec_exp_acos2(T c) {
    constexpr float k[11] = {0.08480516821146011f,  0.26642516255378723f,  0.33367738127708435f,   0.21618370711803436f,
                             0.07947526127099991f,  0.017337322235107422f, 0.0017174964305013418f, -0.00019129738211631775f,
                             0.0007113117026165128f, 0.00020575939561240375f, -0.00034820116707123816f};
    T r = bcv(k[10], c);
#pragma unroll
    for (int i = 9; i >= 0; --i) r = vfma(r, c, bcv(k[i], c));
    return vnan_outside1(c, r);
}

// The light loops of composition.inl:124-160, per light: L = light - pos, one rsqrt gives light_dir and the
// attenuation 1 / distance^2; dot(normalize(light_dir + view_dir), n) with one more rsqrt; the specular
// exp(-acos(x)^2) as one polynomial (spec_exp_acos2). The pixel's view_dir is hoisted out of the loop and the
// frag_color (albedo) factor out of the sum. Within the RGBA16F tolerance of the oracle's libm restatement.
// Light records are wave-uniform (scalar loads from the device globals).
//
// Bounded lights (LB & kLbBounded; soc_composition_bounded): a light with a range r > 0 is multiplied by
// the window w = clamp(1 - (d^2 / r^2)^2, 0, 1), d^2 the dot(l, l) above and 1 / r^2 the upload's rounded reciprocal
// (LightBoundsDev; 0: unlimited, no window and no extra rounding). With f = w for a point light and f = w * cone term for
// a spot light (the cone term alone when unlimited), a light is added to a pixel only where f > 0: a select on the
// accumulator, not a multiply, so a rejected light leaves the pixel's bits untouched whatever its term is (NaN outside a
// spot's cone for a non-unit normal, Inf at d = 0). An unlimited point light is added as in the unbounded form.
// LB & kLbCull: every lane of the wave calls (the unlit ones ride along, as a sky pixel's half does), and the loops walk
// the wave's light masks instead of 0 .. n: mask_of(0 / 1) the point lights 0-63 / 64-127 that may reach a lit pixel of
// the wave, mask_of(2 / 3) the spot lights (composition_pair's cull; each is asked for just before its loop, so one mask
// is live at a time). The index stays scalar, so the records still come through the scalar unit. *ran: lights run.
struct NoMasks {
    __device__ uint64_t operator()(int) const { return 0ull; }
};
__device__ __forceinline__ uint64_t uniform64(uint64_t m) {
    return ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(m >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)m);
}
// composition_pair's cull: lane i's test of light 64 (which & 1) + i against the box of the wave's lit pixels
// (light_cull.hpp: a ranged light by its distance to the box, a spot light also by its outer cone against the box's
// bounding sphere; an unlimited point light always passes), balloted and made provably wave-uniform
struct CullMasks {
    light_cull::Aabb box;
    bool any_lit;   // else every mask is empty
    uint32_t lane, npl, nsl;
    const soc_globals* dg;
    const LightBoundsDev* lb;
    __device__ __forceinline__ uint64_t operator()(int which) const {
        const uint32_t i = 64u * (which & 1) + lane;
        bool keep = false;
        if (which < 2) {
            if (any_lit && i < npl) {
                const float r2 = lb->point_r2[i];
                keep = !(r2 > 0.0f) || !light_cull::sphere_outside_aabb(box, dg->point_lights[i].position, r2);
            }
        } else if (any_lit && i < nsl) {
            const soc_spot_light& L = dg->spot_lights[i];
            const float r2 = lb->spot_r2[i];
            keep = !(r2 > 0.0f && light_cull::sphere_outside_aabb(box, L.position, r2)) &&
                   !light_cull::cone_outside_aabb(box, L.position, L.direction, L.cut_off, L.outer_cut_off);
        }
        return uniform64(__ballot(keep));
    }
};
template <int LB = 0, class T, class MaskOf = NoMasks>
__device__ __forceinline__ V3<T> light_sum(const soc_globals* __restrict__ dg, uint32_t npl, uint32_t nsl, const V3<T>& n,
                                           const V3<T>& pos, f3 cam, const LightBoundsDev* __restrict__ lb = nullptr,
                                           MaskOf mask_of = {}, uint32_t* ran = nullptr) {
    const T z = pos.x;   // lane-type witness for the broadcasts
    const V3<T> vd0 = {bcv(cam.x, z) - pos.x, bcv(cam.y, z) - pos.y, bcv(cam.z, z) - pos.z};
    const T vk = vrsq(vdot(vd0, vd0));
    const V3<T> view_dir = {vd0.x * vk, vd0.y * vk, vd0.z * vk};
    V3<T> acc = {bcv(0.0f, z), bcv(0.0f, z), bcv(0.0f, z)};
    const T nlog2e = bcv(-1.44269504088896f, z);
    T d2;   // the last light's squared distance (the bounded forms' window)
    auto shade_light = [&](const float* lp, T& inv, V3<T>& ld) {
        const V3<T> l = {bcv(lp[0], z) - pos.x, bcv(lp[1], z) - pos.y, bcv(lp[2], z) - pos.z};
        d2 = vdot(l, l);
        inv = vrsq(d2);
        ld = V3<T>{l.x * inv, l.y * inv, l.z * inv};
        const V3<T> h = {ld.x + view_dir.x, ld.y + view_dir.y, ld.z + view_dir.z};
        const T c = vdot(h, n) * vrsq(vdot(h, h));
        const T diffuse = vmax0(vdot(n, ld));
        if (SOC_COMP_SPEC_POLY) return (diffuse + spec_exp_acos2(c)) * (inv * inv);
        const T nh = acos_fast(c);
        return (diffuse + vexp2((nh * nh) * nlog2e)) * (inv * inv);
    };
    // a spot light's cone term (:148-151): the angle to its axis between the outer and the inner cut-off
    auto cone = [&](const soc_spot_light& L, const V3<T>& ld) {
        const float sdx = -L.direction[0], sdy = -L.direction[1], sdz = -L.direction[2];
        const float sk = __builtin_amdgcn_rsqf(__builtin_fmaf(sdz, sdz, __builtin_fmaf(sdy, sdy, sdx * sdx)));
        const T theta = vfma(ld.z, bcv(sdz, z), vfma(ld.y, bcv(sdy, z), ld.x * bcv(sdx, z))) * bcv(sk, z);
        return vclamp01(vdiv(theta - bcv(L.outer_cut_off, z), L.cut_off - L.outer_cut_off));
    };
    auto add = [&](const float* col, T s) {
        acc = V3<T>{vfma(bcv(col[0], z), s, acc.x), vfma(bcv(col[1], z), s, acc.y), vfma(bcv(col[2], z), s, acc.z)};
    };
// 2 lights per round (4: 108 VGPRs, 4 waves per SIMD); with the fused-histogram lights kernel held to 6 waves per SIMD
// (70 VGPRs, no spill): C3b 782 -> 799 fps (profiles/r05_ab_light_loop.txt)
#ifndef SOC_COMP_LIGHT_UNROLL
#define SOC_COMP_LIGHT_UNROLL 2
#endif
    if constexpr (LB != 0) {
        auto add_where = [&](const float* col, T s, T f) {
            acc = V3<T>{vsel_pos(f, vfma(bcv(col[0], z), s, acc.x), acc.x), vsel_pos(f, vfma(bcv(col[1], z), s, acc.y), acc.y),
                        vsel_pos(f, vfma(bcv(col[2], z), s, acc.z), acc.z)};
        };
        auto window = [&](float inv_r2) {
            const T q = d2 * bcv(inv_r2, z);
            return vclamp01(vfma(-q, q, bcv(1.0f, z)));
        };
        auto point = [&](uint32_t i) {
            const soc_point_light& L = dg->point_lights[i];
            const float inv_r2 = lb->point_inv_r2[i];
            T inv;
            V3<T> ld;
            const T s = shade_light(L.position, inv, ld) * bcv(L.intensity, z);
            if (inv_r2 == 0.0f) {   // wave-uniform
                add(L.color, s);
            } else {
                const T w = window(inv_r2);
                add_where(L.color, s * w, w);
            }
        };
        auto spot = [&](uint32_t i) {
            const soc_spot_light& L = dg->spot_lights[i];
            const float inv_r2 = lb->spot_inv_r2[i];
            T inv;
            V3<T> ld;
            const T b = shade_light(L.position, inv, ld);
            T f = cone(L, ld);
            if (inv_r2 != 0.0f) f = window(inv_r2) * f;
            add_where(L.color, b * bcv(L.intensity, z) * f, f);
        };
        if constexpr ((LB & kLbCull) != 0) {
            uint32_t count = 0u;
            auto walk = [&](int which, auto&& light) {
                uint64_t m = mask_of(which);
                count += (uint32_t)__builtin_popcountll(m);
#pragma unroll 1
                for (; m; m &= m - 1) light(64u * (which & 1) + (uint32_t)__builtin_ctzll(m));
            };
            walk(0, point);
            if (npl > 64u) walk(1, point);
            walk(2, spot);
            if (nsl > 64u) walk(3, spot);
            *ran = count;
        } else {
            for (uint32_t i = 0; i < npl; ++i) point(i);
            for (uint32_t i = 0; i < nsl; ++i) spot(i);
        }
        return acc;
    }
#pragma unroll SOC_COMP_LIGHT_UNROLL
    for (uint32_t i = 0; i < npl; ++i) {            // calculate_point_light, :124-139
        const soc_point_light& L = dg->point_lights[i];
        T inv;
        V3<T> ld;
        const T s = shade_light(L.position, inv, ld) * bcv(L.intensity, z);
        add(L.color, s);
    }
#pragma unroll 2
    for (uint32_t i = 0; i < nsl; ++i) {            // calculate_spot_light, :141-160
        const soc_spot_light& L = dg->spot_lights[i];
        T inv;
        V3<T> ld;
        const T b = shade_light(L.position, inv, ld);
        const T intensity = cone(L, ld);
        add(L.color, b * bcv(L.intensity, z) * intensity);
    }
    return acc;
}

// Shading of one pixel given its G-buffer values (composition.inl:164-224), in two parts around the light sum:
// shade_pre (sun ESM shadow, emissive, AO) and shade_post (lights, ambient, albedo, AO, emissive).
// The sun-space position is one projective transform of the NDC point: vs = inv_proj * ndc,
// ws = inv_view * (vs / vs.w), sp = sun_pv * ws, and pc = sp.xyz / sp.w, so the vs.w division cancels
// and sun_clip = sun_pv * inv_view * inv_proj (host fp32) gives pc directly (one rcp; within the
// RGBA16F tolerance). The world position itself is only formed for the light loops.
struct ShadePre {
    float direct;   // the sun term dot(n, -sun) * shadow (grey)
    float occl;
    f3 em;
};
// shade_pre without the shadow: direct = dot(n, -sun), to be multiplied by the sun's shadow term (here, or cascade_shadow)
__device__ __forceinline__ ShadePre shade_pre_unshadowed(const CompParams& p, f3 emissive, f3 n, float ssao) {
    ShadePre s;
    s.em = emissive * p.emissive_strength;
    s.occl = fast_pow(ssao, p.ao_strength);
    s.direct = fmaxf(0.0f, dot3(n, -mk3(p.sun_dir[0], p.sun_dir[1], p.sun_dir[2])));
    return s;
}
template <typename ShadowImg = DImg>
__device__ __forceinline__ ShadePre shade_pre(const CompParams& p, float u, float v, float d, f3 emissive, f3 n, float ssao,
                                              const ShadowImg& shadow) {
    const f4 ndc = f4{u * 2.0f - 1.0f, v * 2.0f - 1.0f, d, 1.0f};
    // sun ESM shadow, :166-173
    const f4 sp = mul(p.sun_clip, ndc);
    const float rsw = __builtin_amdgcn_rcpf(sp.w);
    const float pcx = sp.x * rsw * 0.5f + 0.5f;
    const float pcy = sp.y * rsw * 0.5f + 0.5f;
    const float pcz = sp.z * rsw;
    const float sd = (SOC_COMP_PROFILE & 1) ? pcx * 0.001f : sample_f32(shadow, pcx, pcy);
    float e = __expf(p.ef * (pcz - sd));
    if (p.df != 1.0f) e = fast_pow(e, p.df);   // pow(x, 1.0) == x exactly
    const float sun_shadow = clampf(e, 0.0f, 1.0f);
    ShadePre s = shade_pre_unshadowed(p, emissive, n, ssao);
    s.direct *= sun_shadow;
    return s;
}
// get_world_position_from_depth, :114-122
__device__ __forceinline__ f3 world_pos(const CompParams& p, float u, float v, float d) {
    const f4 ndc = f4{u * 2.0f - 1.0f, v * 2.0f - 1.0f, d, 1.0f};
    f4 vs = mul(p.inv_proj, ndc);
    const float rw = __builtin_amdgcn_rcpf(vs.w);
    vs = f4{vs.x * rw, vs.y * rw, vs.z * rw, 1.0f};
    const f4 ws = mul(p.inv_view, vs);
    return f3{ws.x, ws.y, ws.z};
}
__device__ __forceinline__ f4 shade_post(const CompParams& p, const ShadePre& s, f3 albedo, const f3* lights) {
    f3 direct = f3{s.direct, s.direct, s.direct};
    if (lights)
        direct = f3{__builtin_fmaf(albedo.x, lights->x, direct.x), __builtin_fmaf(albedo.y, lights->y, direct.y),
                    __builtin_fmaf(albedo.z, lights->z, direct.z)};
    const f3 c = (direct + mk3(p.ambient[0], p.ambient[1], p.ambient[2])) * albedo * s.occl + s.em;
    return f4{c.x, c.y, c.z, 1.0f};
}
template <bool LIGHTS = true, typename ShadowImg = DImg, int LB = 0>
__device__ __forceinline__ f4 shade(const CompParams& p, float u, float v, float d, f3 albedo, f3 emissive, f3 n,
                                    float ssao, const ShadowImg& shadow, const LightBoundsDev* lb = nullptr) {
    const ShadePre s = shade_pre(p, u, v, d, emissive, n, ssao, shadow);
    if (LIGHTS && (p.npl | p.nsl)) {
        const f3 wp = world_pos(p, u, v, d);
        const V3<float> ls = light_sum<LB>(p.dg, p.npl, p.nsl, V3<float>{n.x, n.y, n.z}, V3<float>{wp.x, wp.y, wp.z},
                                           mk3(p.cam[0], p.cam[1], p.cam[2]), lb);
        const f3 l3 = f3{ls.x, ls.y, ls.z};
        return shade_post(p, s, albedo, &l3);
    }
    return shade_post(p, s, albedo, nullptr);
}

// Fast path: all full-res images share the target extent, width even, rows 16-B aligned.
// HIST: GenerateLuminanceHistogramTask fused in (generate_luminance_histogram.inl:59-78): the bins of the
// two stored RGBA16F pixels (the exact values the histogram pass would read back; lum_bin_fast with the
// exact fallback) are added into the wave's LDS histogram with one LDS atomic per lane (lane_bin_pair_mask: measured 90 -> 66 us
// at 4K on the textured mesh against the ballot-aggregated loop, whose rounds grow with the distinct bins of a wave and
// run on the VALU), which the workgroup flushes with one device atomic per
// non-zero bin (~3.6 distinct bins per 32x16 tile at 4K), saving the 8 B/px re-read of the colour.
// The flush goes to one of 8 scratch copies chosen by linear block id mod 8 (the XCD under round-robin
// dispatch): a single copy serialises the ~5k atomics of the hottest bin (measured 172 us vs 77 us),
// 8 copies cut that 8x. histogram_fold adds the copies into the AutoExposure bins and re-zeroes them.
// Measured at 4K (kernel trace): 68.4 us + a 4 us fold against 66-68 + 27.7 us for the two passes; frame
// 0.679 -> 0.660 ms. The render graph fuses by default (SOC_RENDERER_UNFUSED_HISTOGRAM: two passes).
// (An in-kernel fold by the last-arriving workgroup instead of the fold launch costs one same-address
// device atomic per workgroup: 16,200 of them serialise across the XCDs, 68 -> 207 us.)
// LIGHTS = false: no point / spot lights this frame (the reference default): the light loops are not
// compiled in, which keeps the kernel at a fraction of the registers (more waves, more loads in flight).
// BL (SOC_RENDERER_BLOOM_IN_COMPOSITION): the bloom chain's last upsample pair (mip1 -> [mip0] -> output, bloomw_up10s)
// is computed for the workgroup's 32 x 16 tile in LDS (Up10Tile, bloom_w.hpp: the same values per pixel, rounded to
// RGBA16F as the chain stores its output) while the G-buffer loads are in flight, and used as the emissive input, so
// the full-resolution bloom output is neither written by the chain nor read back here (16 B/px). `emissive` unused.
// p.bloom_sparse (SOC_BLOOM_SPARSE, the render graph only): the workgroup's 32 x 16 tile is a cell of bloom_w.hpp; each
// wave tests the cell's mip3 footprint itself (no LDS, no barrier; the four waves load the same texels and agree). In a
// proven cell the bloom is pack3(+0, +0, +0) without the `emissive` load (the sparse last stage left those pixels
// unwritten) or, with BL, without the mip1 tile and its barriers; any other cell runs as without the flag.
#ifndef SOC_COMP_LIGHT_WAVES
#define SOC_COMP_LIGHT_WAVES 6
#endif
// LB (0: the kernels as they were, same signature, same instructions: profiles/light_bounds_isa_identity.txt; else the
// parameter block is CompParamsBounded): the bounded lights of light_sum, in instantiations of their own.
// kLbCull: before the loops each wave reduces the world-space box of its lit pixels (sky, out-of-image and, in the
// kernels without the histogram, the lanes that would have left: +-inf), lane i tests lights i and i + 64 of each kind
// against it (light_cull.hpp: a ranged light by its distance to the box, a spot light also by its outer cone against the
// box's bounding sphere; an unlimited point light always passes), and the ballots, made provably wave-uniform, are the
// masks the loops walk. A wave without a lit pixel has empty masks. kLbCount: the wave adds the number of lights its
// loops run to *la.shaded (the measuring calls only: one same-address atomic per wave).
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
// Cascaded sun shadows (CS; soc_composition_cascaded), in instantiations of their own with a parameter
// block of their own: `shadow` is the atlas (S x count * S, cascade c = rows [c * S, (c + 1) * S)), pv[c] the cascade's
// projection_view (world -> sun clip space), ef[c] its ESM factor, split[] the stored depths that separate the cascades
// (+inf from count - 1 on, so the compares need no count).
//
// The pixel's sun-space position and its tap position are computed in fp64, from the same fp32 matrix entries, depth and
// pixel centre the fp32 kernels use. The fitted cascades keep the sun's softness in WORLD units, so ef[c] grows with the
// cascade's depth range (-1000 .. -2500 for slices 50 - 200 units wide, against the sun's -80), and the exponent
// ef * (z - d) magnifies what fp32 leaves of a position 100 units away:
//  - shade_pre's combined matrix (sun_pv * inv_view * inv_proj in host fp32) has entries of magnitude 5 (inv_proj's w row
//    is about -5 d + 5) whose sum is 1 / distance: exponent errors of 0.01 - 0.1 on the test frames, 2 - 20 times the
//    RGBA16F tolerance (fp32 on the CPU against the float64 oracle);
//  - through the world position with w = fma(m11, d, m15) the exponent holds to 2e-4, but the tap's 8-bit sub-texel
//    weight (floor(t * 256 + 0.5), the sampling contract) then still rounds the other way than the oracle's on about one
//    pixel in a thousand (fp32 leaves 1e-3 of a weight step at t = 128 texels), and one weight step between texels a
//    world unit apart in depth is 0.02 in the exponent: single pixels 1.2 and 2.2 tolerances off in two of six frames.
// In fp64 both vanish (the position agrees with the oracle's to 1e-12 of a weight step). The price is about 45 fp64 fmas
// and two divisions per lit pixel (DESIGN.md §5.8 has the timings); the G-buffer, the AO tap and the lights stay fp32.
struct d3 { double x, y, z; };
// the cascade of a stored depth: the number of splits below it (a NaN depth compares false: cascade 0)
__device__ __forceinline__ int cascade_of(const CompParamsCascaded& p, float d) {
    return (d > p.split[0] ? 1 : 0) + (d > p.split[1] ? 1 : 0) + (d > p.split[2] ? 1 : 0);
}
// M * (x, y, z, 1) -> xyz, w
__device__ __forceinline__ d3 mul_point(const Mat4d& M, double x, double y, double z, double& w) {
    const double* m = M.m;
    w = __builtin_fma(m[3], x, __builtin_fma(m[7], y, __builtin_fma(m[11], z, m[15])));
    return d3{__builtin_fma(m[0], x, __builtin_fma(m[4], y, __builtin_fma(m[8], z, m[12]))),
              __builtin_fma(m[1], x, __builtin_fma(m[5], y, __builtin_fma(m[9], z, m[13]))),
              __builtin_fma(m[2], x, __builtin_fma(m[6], y, __builtin_fma(m[10], z, m[14])))};
}
// get_world_position_from_depth (:114-122) of pixel (x, y) with stored depth d, for the cascades' shadow lookup
__device__ __forceinline__ d3 world_d(const CompParamsCascaded& p, int x, int y, float d) {
    const double u = ((double)x + 0.5) * p.rw_d, v = ((double)y + 0.5) * p.rh_d;
    double vw, ww;
    const d3 vs = mul_point(p.inv_proj_d, __builtin_fma(u, 2.0, -1.0), __builtin_fma(v, 2.0, -1.0), (double)d, vw);
    const double r = 1.0 / vw;
    return mul_point(p.inv_view_d, vs.x * r, vs.y * r, vs.z * r, ww);
}
// axis_clamp (soc_device.hpp) on a coordinate held in fp64: the same taps and 8-bit weight
__device__ __forceinline__ Axis axis_clamp_d(double u, int n) {
    double t = u * (double)n - 0.5;
    t = fmin(fmax(t, -2.0), (double)n + 1.0);
    const int fx = (int)floor(t * 256.0 + 0.5);
    int i = fx >> 8;
    float w = (float)(fx & 255) * (1.0f / 256.0f);
    if (i < 0) { i = 0; w = 0.0f; }
    else if (i >= n - 1) { i = n - 2; w = 1.0f; }
    Axis a;
    a.i0 = i;
    a.i1 = i + 1;   // n >= 2 (validated)
    a.w = w;
    return a;
}
// sample_f32 on the S x S slab whose first row is row0: the taps and weights of the slab alone (clamp-to-edge stays
// inside it), the rows then offset
__device__ __forceinline__ float sample_f32_slab(const BufImg& b, double u, double v, int S, int row0) {
    typedef float f2u4 __attribute__((ext_vector_type(2))) __attribute__((aligned(4)));
    const Axis ax = axis_clamp_d(u, S), ay = axis_clamp_d(v, S);
    const int o = ax.i0 * 4;
    const f2u4 r0 = __builtin_bit_cast(f2u4, __builtin_amdgcn_raw_buffer_load_b64(b.r, buf_row(b, row0 + ay.i0) + o, 0, 0));
    const f2u4 r1 = __builtin_bit_cast(f2u4, __builtin_amdgcn_raw_buffer_load_b64(b.r, buf_row(b, row0 + ay.i1) + o, 0, 0));
    return bilerp1(r0.x, r0.y, r1.x, r1.y, ax.w, ay.w);
}
__device__ __forceinline__ float sample_f32_slab(const DImg& im, double u, double v, int S, int row0) {
    const Axis ax = axis_clamp_d(u, S), ay = axis_clamp_d(v, S);
    const soc_f2a4 p0 = *reinterpret_cast<const soc_f2a4*>(row_ptr<float>(im, row0 + ay.i0) + ax.i0);
    const soc_f2a4 p1 = *reinterpret_cast<const soc_f2a4*>(row_ptr<float>(im, row0 + ay.i1) + ax.i0);
    return bilerp1(p0.x, p0.y, p1.x, p1.y, ax.w, ay.w);
}
// The sun ESM shadow (:166-173) of the world position w in cascade c (wave-uniform: the matrix comes through the scalar
// unit): project, one tap inside slab c, the exponential with the cascade's factor in fp32 as shade_pre has it.
template <typename ShadowImg>
__device__ __forceinline__ float cascade_shadow(const CompParamsCascaded& p, int c, const d3& w, const ShadowImg& shadow) {
    double sw;
    const d3 sp = mul_point(p.pv[c], w.x, w.y, w.z, sw);
    const double r = 1.0 / sw;
    const float pcz = (float)(sp.z * r);
    const float sd = sample_f32_slab(shadow, __builtin_fma(sp.x * r, 0.5, 0.5), __builtin_fma(sp.y * r, 0.5, 0.5), p.S, c * p.S);
    float e = __expf(p.ef[c] * (pcz - sd));
    if (p.df != 1.0f) e = fast_pow(e, p.df);   // pow(x, 1.0) == x exactly
    return clampf(e, 0.0f, 1.0f);
}
// The sun shadows of up to NPX pixels of a lane, each with its own cascade ck[i] (live[i]: the pixel is lit) and world
// position. The wave walks the cascades: one that no live pixel of the wave selects is skipped (wave-uniform branch),
// the others run cascade_shadow under the mask of the lanes that selected them. A wave whose pixels share one cascade
// (the common case on 16 x 8 patches) runs one round; a mixed wave one round per cascade present. A pixel's arithmetic
// is the same in either case and involves no other lane's values, so its bits do not depend on the wave it is in.
template <int NPX, typename ShadowImg>
__device__ __forceinline__ void cascade_shadows(const CompParamsCascaded& p, const bool* live, const int* ck, const d3* w,
                                                const ShadowImg& shadow, float* out) {
#pragma unroll 1
    for (int c = 0; c < p.count; ++c) {
        bool mine[NPX], any = false;
#pragma unroll
        for (int i = 0; i < NPX; ++i) {
            mine[i] = live[i] && ck[i] == c;
            any = any || mine[i];
        }
        if (__ballot(any) == 0ull) continue;
#pragma unroll
        for (int i = 0; i < NPX; ++i)
            if (mine[i]) out[i] = cascade_shadow(p, c, w[i], shadow);
    }
}
// The fused histogram's tail, by every lane of the workgroup: the bins of the lane's two stored pixels (mask: the pixels this
// kernel wrote; lum_bin_fast with the exact fallback) into the wave's LDS histogram `sh + wave * kBins`, then the
// workgroup's four histograms into one of the 8 scratch copies (linear block id mod 8), one device atomic per non-zero bin.
__device__ __forceinline__ void bin_pair_and_flush(uint32_t* sh, int wave, const uint2* outp, uint32_t mask, const CompParams& p) {
    const f4 c0 = unpack_h4(outp[0]), c1 = unpack_h4(outp[1]);
    uint32_t b0 = lum_bin_fast(c0.x, c0.y, c0.z, p.bf);
    uint32_t b1 = lum_bin_fast(c1.x, c1.y, c1.z, p.bf);
    if (b0 == kBinExact) b0 = lum_bin(c0.x, c0.y, c0.z, p.lmin, p.lrange);
    if (b1 == kBinExact) b1 = lum_bin(c1.x, c1.y, c1.z, p.lmin, p.lrange);
    lane_bin_pair_mask(sh + wave * kBins, b0, b1, mask);
    __syncthreads();
    const uint32_t n = sh[threadIdx.x] + sh[kBins + threadIdx.x] + sh[2 * kBins + threadIdx.x] + sh[3 * kBins + threadIdx.x];
    if (n) atomicAdd(&p.bins[((blockIdx.y * gridDim.x + blockIdx.x) & 7u) * kBins + threadIdx.x], n);
}
template <bool HIST, bool LIGHTS, int NT = 0, bool BL = false, bool SP = false, int LB = 0, bool CS = false>
__global__ __launch_bounds__(kWorkgroup) __attribute__((amdgpu_waves_per_eu(LIGHTS && !BL ? SOC_COMP_LIGHT_WAVES : 1))) void composition_pair(DImg target, DImg albedo, DImg emissive, DImg normal, DImg depth,
                                                        DImg ssao, DImg shadow, DImg clouds,
                                                        std::conditional_t<CS, CompParamsCascaded, std::conditional_t<LB != 0, CompParamsBounded, CompParams>> p, DImg mip1, DImg mip3) {
    static_assert(!SP || ((LIGHTS || BL) && HIST), "SP: the LIGHTS / BL kernels' form of p.bloom_sparse (the render graph's launches)");
    static_assert(LB == 0 || (LIGHTS && (LB & kLbBounded)), "LB: forms of the lights kernels");
    static_assert(!CS || (LB == 0 && !BL && !SP), "CS: cascades come without bounded lights, in-kernel bloom and zero cells");
    static_assert(!(LB & kLbCount) || (!BL && !SP), "the counting forms are the stand-alone calls'");
    constexpr bool CULL = (LB & kLbCull) != 0;
    LightArgs la = {};
    if constexpr (LB != 0) la = p.la;
    static_assert(!BL || HIST, "the in-kernel bloom runs in the fused-histogram kernel (no early exit before its barriers)");
    // a wave covers 16x8 pixels (8 lanes x 2 pixels per row, 8 rows): every row segment is one
    // 128-B line of each G-buffer image, and the wave's shadow-map taps form a compact 2D patch
    // (a 128x1 strip maps to a line across the 4096^2 map and touches a new line per tap)
    // HIST: one 256-bin LDS histogram per wave, zeroed by its own wave (LDS operations of a wave are
    // ordered), so no barrier stands in front of the G-buffer loads
    __shared__ uint32_t sh[HIST ? 4 * kBins : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (HIST) reinterpret_cast<uint4*>(sh + wave * kBins)[lane] = uint4{0u, 0u, 0u, 0u};
    int bx, by;
    xcd_order(p.swz, bx, by);
    const int x = bx * 32 + (wave & 1) * 16 + (lane & 7) * 2;
    const int y = by * 16 + (wave >> 1) * 8 + (lane >> 3);
    const bool inside = x < target.w && y < target.h;
    static_assert(kCellW == 32 && kCellH == 16, "the workgroup's tile is the bloom's cell");
    // the cell's mip3 taps, issued ahead of the G-buffer loads; the vote that waits for them follows those loads
    // (the lights and in-kernel-bloom kernels take the flag as the template parameter SP: the runtime branch cost them
    // registers, and occupancy with them; HIST: the render graph's launches, where no lane leaves before the vote)
    const bool prove = HIST && ((LIGHTS || BL) ? SP : p.bloom_sparse != 0);   // wave-uniform
    ZeroCellTaps<1> zt = {};
    if (prove) zero_cells_load<1>(mip3, bx, bx, by, lane, zt);
    // the lights kernels vote at once: the taps held across the G-buffer loads cost them registers they do not have
    bool bloom_zero = false;
    if (LIGHTS && prove) bloom_zero = zero_cells_vote<1, false>(zt);
    if (!HIST && !CULL && !inside) return;   // CULL: every lane stays for the wave's reduction (neutral, no access)
    uint2 outp[2] = {uint2{0u, 0u}, uint2{0u, 0u}};
    uint32_t own = 3u;   // bit k: this kernel writes (and bins) pixel k of the pair
    // buffer descriptors + 32-bit offsets (one multiply-add per image row instead of 64-bit pointer math)
    const BufImg bd = buf_img(depth), ba = buf_img(albedo), be = buf_img(emissive), bn = buf_img(normal);
    const BufImg bt = buf_img(target), bs = buf_img(shadow), bo = buf_img(ssao);
    const float v = centre_uv_rn(y, target.h, p.rh);
    // once-read streams non-temporal (NT & 1: keep L2 for the shadow-map / AO gathers); aux bit 1 = nt
    constexpr int ld_aux = (NT & 1) ? 2 : 0;
    float2 d2 = float2{0.0f, 0.0f};
    uint4 a4 = uint4{0u, 0u, 0u, 0u}, n4 = a4;
    const uint2 bz = pack3(C3{0.0f, 0.0f, 0.0f});
    uint4 e4 = uint4{bz.x, bz.y, bz.x, bz.y};   // the bloom of a proven cell, unless loaded (or computed, BL) below
    // NT & 4: both pixels' AO taps (3 half-res texels per row) as one 8-B load per row, issued with the G-buffer
    // loads (not after the depth test), for sky pixels too (in bounds, unused); the same bits as sample_r8
    float aop[2] = {0.0f, 0.0f};
    if (inside) {
        d2 = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(bd.r, buf_row(bd, y) + x * 4, 0, ld_aux));
        a4 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(ba.r, buf_row(ba, y) + x * 8, 0, ld_aux));
        if (!BL && (LIGHTS ? !bloom_zero : !prove)) e4 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(be.r, buf_row(be, y) + x * 8, 0, ld_aux));
        n4 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(bn.r, buf_row(bn, y) + x * 8, 0, ld_aux));
        if (NT & 4) sample_r8_pair(bo, centre_uv_rn(x, target.w, p.rw), centre_uv_rn(x + 1, target.w, p.rw), v, aop[0], aop[1]);
    }
    // wave-uniform, by all 64 lanes; the emissive load it decides comes one latency after the others in an unproven cell
    if (!LIGHTS && prove) bloom_zero = zero_cells_vote<1>(zt);
    if (!BL && !LIGHTS && prove && !bloom_zero && inside)
        e4 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(be.r, buf_row(be, y) + x * 8, 0, ld_aux));
    if constexpr (BL) {   // every lane takes part in the tile's barriers; the pair's bloom as the chain stores it
        __shared__ Up10Tile<32, 16> bl;
        const int X0 = bx * 32, Y0 = by * 16;
        // a proven cell (workgroup-uniform: every wave computed the same proof, so none reaches build's barriers), or an
        // all-zero mip1 tile (SOC_BLOOM_ZERO_SKIP): the pair is pack3(+0, +0, +0) without the tile's sums
        if (!bloom_zero && !bl.build(mip1, X0, Y0, target.w, target.h, threadIdx.x, p.bloom_zero_skip != 0)) {
            C3 o[2];
            bl.out(y - Y0, x - X0, o);
            const uint2 b0 = pack3(o[0]), b1 = pack3(o[1]);
            e4 = uint4{b0.x, b0.y, b1.x, b1.y};
        }
    }
    if (CULL || inside) {
        // LIGHTS: the light sum of the lane's two pixels runs once, as packed pairs (light_sum<f2v>, the same bits per
        // pixel as light_sum<float>); a sky pixel of the pair rides along in the other half and is discarded
        ShadePre pre[2];
        f3 alb[2], nrm[2], wps[2];
        if constexpr (CULL) nrm[0] = nrm[1] = wps[0] = wps[1] = f3{0.0f, 0.0f, 0.0f};   // a lane outside the image rides along
        uint32_t lit = 0u;
        [[maybe_unused]] d3 cw[2] = {d3{0.0, 0.0, 0.0}, d3{0.0, 0.0, 0.0}};           // CS: a lit pixel's world position
        [[maybe_unused]] int ck[2] = {0, 0};                                          // ... and its cascade
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (CULL && !inside) continue;   // stays unlit and unwritten
            const float u = centre_uv_rn(x + k, target.w, p.rw);
            const float d = k ? d2.y : d2.x;
            const f4 al = unpack_h4(k ? uint2{a4.z, a4.w} : uint2{a4.x, a4.y});
            const f4 em = unpack_h4(k ? uint2{e4.z, e4.w} : uint2{e4.x, e4.y});
            const f4 nn = unpack_h4(k ? uint2{n4.z, n4.w} : uint2{n4.x, n4.y});
            f4 c;
            if (LIGHTS) {   // the same pixel values for a sky pixel's discarded half
                nrm[k] = f3{nn.x, nn.y, nn.z};
                wps[k] = world_pos(p, u, v, d);
            }
            if (d == 1.0f && p.sky_external) {   // the second lane writes it (sky_compose_pair)
                own &= ~(1u << k);
                continue;
            }
            if (d == 1.0f) {
                const f4 cl = fetch_rgba8(clouds, x + k, y);
                c = f4{cl.x, cl.y, cl.z, 1.0f};
            } else {
                const float ao = (SOC_COMP_PROFILE & 2) ? u : (NT & 4) ? aop[k] : sample_r8(bo, u, v);
                if constexpr (CS) {   // the shadow follows below, cascade by cascade for the whole wave
                    pre[k] = shade_pre_unshadowed(p, f3{em.x, em.y, em.z}, f3{nn.x, nn.y, nn.z}, ao);
                    alb[k] = f3{al.x, al.y, al.z};
                    cw[k] = world_d(p, x + k, y, d);
                    ck[k] = cascade_of(p, d);
                    lit |= 1u << k;
                    continue;
                }
                if (LIGHTS) {
                    pre[k] = shade_pre(p, u, v, d, f3{em.x, em.y, em.z}, f3{nn.x, nn.y, nn.z}, ao, bs);
                    alb[k] = f3{al.x, al.y, al.z};
                    lit |= 1u << k;
                    continue;
                }
                c = shade<false>(p, u, v, d, f3{al.x, al.y, al.z}, f3{em.x, em.y, em.z}, f3{nn.x, nn.y, nn.z}, ao, bs);
            }
            outp[k] = pack_h4(c);
        }
        if constexpr (CS) {
            const bool live[2] = {(lit & 1u) != 0u, (lit & 2u) != 0u};
            float sun[2] = {0.0f, 0.0f};
            cascade_shadows<2>(p, live, ck, cw, bs, sun);
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (live[k]) {
                    pre[k].direct *= sun[k];
                    if (!LIGHTS) outp[k] = pack_h4(shade_post(p, pre[k], alb[k], nullptr));
                }
        }
        // CULL, all 64 lanes here: the box of the wave's lit pixels (fminf drops a NaN coordinate: such a pixel fails every
        // bounded light's own test as well)
        std::conditional_t<CULL, CullMasks, NoMasks> mask_of = {};
        if constexpr (CULL) {
            constexpr float kInf = __builtin_inff();
            auto lo = [&](float w0, float w1) { return wave_min(fminf((lit & 1u) ? w0 : kInf, (lit & 2u) ? w1 : kInf)); };
            mask_of.box = light_cull::Aabb{lo(wps[0].x, wps[1].x),     lo(wps[0].y, wps[1].y),     lo(wps[0].z, wps[1].z),
                                           -lo(-wps[0].x, -wps[1].x), -lo(-wps[0].y, -wps[1].y), -lo(-wps[0].z, -wps[1].z)};
            mask_of.any_lit = __ballot(lit != 0u) != 0ull;
            mask_of.lane = (uint32_t)lane;
            mask_of.npl = p.npl;
            mask_of.nsl = p.nsl;
            mask_of.dg = p.dg;
            mask_of.lb = la.lb;
        }
        if constexpr (!CULL && (LB & kLbCount) != 0) {   // the lanes inside the image: the first of them counts
            const uint64_t here = __ballot(true);
            if (__ballot(lit != 0u) != 0ull && lane == __builtin_ctzll(here)) atomicAdd(la.shaded, p.npl + p.nsl);
        }
        bool sum_lights = lit != 0u;
        if constexpr (CULL) sum_lights = mask_of.any_lit;   // wave-uniform: all lanes or none
        if (LIGHTS && sum_lights) {
            uint32_t ran = 0u;
            const V3<f2v> n2 = {f2v{nrm[0].x, nrm[1].x}, f2v{nrm[0].y, nrm[1].y}, f2v{nrm[0].z, nrm[1].z}};
            const V3<f2v> w2 = {f2v{wps[0].x, wps[1].x}, f2v{wps[0].y, wps[1].y}, f2v{wps[0].z, wps[1].z}};
            const V3<f2v> ls = light_sum<LB>(p.dg, p.npl, p.nsl, n2, w2, mk3(p.cam[0], p.cam[1], p.cam[2]), la.lb, mask_of, &ran);
            if constexpr (CULL && (LB & kLbCount) != 0)
                if (lane == 0 && ran) atomicAdd(la.shaded, ran);
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (lit & (1u << k)) {
                    const f3 l3 = k ? f3{ls.x.y, ls.y.y, ls.z.y} : f3{ls.x.x, ls.y.x, ls.z.x};
                    outp[k] = pack_h4(shade_post(p, pre[k], alb[k], &l3));
                }
        }
        const uint4 o = uint4{outp[0].x, outp[0].y, outp[1].x, outp[1].y};
        typedef uint32_t v4w __attribute__((ext_vector_type(4)));
        const int to = buf_row(bt, y) + x * 8;
        if (CULL && !inside) own = 0u;   // nothing to store
        if (own == 3u) {
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4w, o), bt.r, to, 0, (NT & 2) ? 2 : 0);
        } else {   // a sky pixel in the pair belongs to the second lane: 8-B stores of ours only
            typedef uint32_t v2w __attribute__((ext_vector_type(2)));
            if (own & 1u) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2w, outp[0]), bt.r, to, 0, 0);
            if (own & 2u) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2w, outp[1]), bt.r, to + 8, 0, 0);
        }
    }
    if (HIST) bin_pair_and_flush(sh, wave, outp, inside ? own : 0u, p);
}
// The sky pixels of the colour image (composition.inl:220-222: depth == 1 -> color = clouds texel), written and
// binned on the renderer's second lane right after CloudRendering, so Composition (sky_external) does not wait
// for the clouds: the same tiling, texel fetch, f16 packing and bins as composition_pair's sky branch, hence
// the same bits. 8-B stores of the sky pixels only (Composition writes the others concurrently).
// CP (clouds rows 8-B aligned): a pair's two clouds texels in one 8-B load, issued once the depth shows a sky pixel in
// the pair (one dependent load level instead of two); else the per-pixel form. The same texels.
template <bool CP>
__global__ __launch_bounds__(kWorkgroup) void sky_compose_pair(DImg target, DImg depth, DImg clouds, CompParams p) {
    __shared__ uint32_t sh[4 * kBins];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    reinterpret_cast<uint4*>(sh + wave * kBins)[lane] = uint4{0u, 0u, 0u, 0u};
    const int bx = blockIdx.x, by = blockIdx.y;
    const int x = bx * 32 + (wave & 1) * 16 + (lane & 7) * 2;
    const int y = by * 16 + (wave >> 1) * 8 + (lane >> 3);
    const bool inside = x < target.w && y < target.h;
    uint32_t mine = 0u;
    uint2 outp[2] = {uint2{0u, 0u}, uint2{0u, 0u}};
    if (inside) {
        const float2 d2 = row_ptr<float2>(depth, y)[x >> 1];
        const bool s0 = d2.x == 1.0f, s1 = d2.y == 1.0f;
        if (!CP) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (!(k ? s1 : s0)) continue;
                const f4 cl = fetch_rgba8(clouds, x + k, y);
                outp[k] = pack_h4(f4{cl.x, cl.y, cl.z, 1.0f});
                row_ptr_w<uint2>(target, y)[x + k] = outp[k];
                mine |= 1u << k;
            }
        } else if (s0 || s1) {   // both clouds texels of the pair in one 8-B load (the pair's x is even)
            const uint2 cw = row_ptr<uint2>(clouds, y)[x >> 1];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (!(k ? s1 : s0)) continue;
                const f4 cl = unpack_rgba8(k ? cw.y : cw.x);
                outp[k] = pack_h4(f4{cl.x, cl.y, cl.z, 1.0f});
                row_ptr_w<uint2>(target, y)[x + k] = outp[k];
                mine |= 1u << k;
            }
        }
    }
    bin_pair_and_flush(sh, wave, outp, mine, p);
}

__global__ __launch_bounds__(kBins) void histogram_fold(uint32_t* __restrict__ scratch, uint32_t* __restrict__ bins) {
    const int i = threadIdx.x;
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        s += scratch[k * kBins + i];
        scratch[k * kBins + i] = 0u;
    }
    if (s) bins[i] += s;
}

// Generic path: every input is sampled under the sampling contract.
template <int LB>
__device__ __forceinline__ void composition_generic_body(const DImg& target, const DImg& albedo, const DImg& emissive, const DImg& normal,
                                                         const DImg& depth, const DImg& ssao, const DImg& shadow, const DImg& clouds,
                                                         const CompParams& p, const LightBoundsDev* lb) {
    const int x = blockIdx.x * kGenericBlockX + threadIdx.x, y = blockIdx.y * kGenericBlockY + threadIdx.y;
    if (x >= target.w || y >= target.h) return;
    const float u = centre_uv(x, target.w), v = centre_uv(y, target.h);
    const float d = sample_f32(depth, u, v);
    f4 c;
    if (d == 1.0f) {
        const f4 cl = sample_rgba8(clouds, u, v);
        c = f4{cl.x, cl.y, cl.z, 1.0f};
    } else {
        const f4 al = sample_h4(albedo, u, v), em = sample_h4(emissive, u, v), nn = sample_h4(normal, u, v);
        c = shade<true, DImg, LB>(p, u, v, d, f3{al.x, al.y, al.z}, f3{em.x, em.y, em.z}, f3{nn.x, nn.y, nn.z}, sample_r8(ssao, u, v),
                                  shadow, lb);
    }
    row_ptr_w<uint2>(target, y)[x] = pack_h4(c);
}
__global__ __launch_bounds__(kWorkgroup) void composition_generic(DImg target, DImg albedo, DImg emissive, DImg normal,
                                                           DImg depth, DImg ssao, DImg shadow, DImg clouds, CompParams p) {
    composition_generic_body<0>(target, albedo, emissive, normal, depth, ssao, shadow, clouds, p, nullptr);
}
// bounded lights, every pixel by its own test (no wave patches here: no cull and no count)
__global__ __launch_bounds__(kWorkgroup) void composition_generic_bounded(DImg target, DImg albedo, DImg emissive, DImg normal,
                                                           DImg depth, DImg ssao, DImg shadow, DImg clouds, CompParams p,
                                                           const LightBoundsDev* lb) {
    composition_generic_body<kLbBounded>(target, albedo, emissive, normal, depth, ssao, shadow, clouds, p, lb);
}

// cascaded sun shadows off the pair path: a pixel per lane, the wave's cascades walked as in composition_pair
__global__ __launch_bounds__(kWorkgroup) void composition_generic_cascaded(DImg target, DImg albedo, DImg emissive, DImg normal,
                                                           DImg depth, DImg ssao, DImg shadow, DImg clouds, CompParamsCascaded p) {
    const int x = blockIdx.x * kGenericBlockX + threadIdx.x, y = blockIdx.y * kGenericBlockY + threadIdx.y;
    if (x >= target.w || y >= target.h) return;
    const float u = centre_uv(x, target.w), v = centre_uv(y, target.h);
    const float d = sample_f32(depth, u, v);
    const bool live = !(d == 1.0f);
    const int ck = cascade_of(p, d);
    const d3 w = world_d(p, x, y, d);
    float sun = 0.0f;
    cascade_shadows<1>(p, &live, &ck, &w, shadow, &sun);
    f4 c;
    if (!live) {
        const f4 cl = sample_rgba8(clouds, u, v);
        c = f4{cl.x, cl.y, cl.z, 1.0f};
    } else {
        const f4 al = sample_h4(albedo, u, v), em = sample_h4(emissive, u, v), nn = sample_h4(normal, u, v);
        ShadePre s = shade_pre_unshadowed(p, f3{em.x, em.y, em.z}, f3{nn.x, nn.y, nn.z}, sample_r8(ssao, u, v));
        s.direct *= sun;
        if (p.npl | p.nsl) {   // shade<true>'s lights
            const f3 wp = world_pos(p, u, v, d);
            const V3<float> ls = light_sum<0>(p.dg, p.npl, p.nsl, V3<float>{nn.x, nn.y, nn.z}, V3<float>{wp.x, wp.y, wp.z},
                                              mk3(p.cam[0], p.cam[1], p.cam[2]));
            const f3 l3 = f3{ls.x, ls.y, ls.z};
            c = shade_post(p, s, f3{al.x, al.y, al.z}, &l3);
        } else {
            c = shade_post(p, s, f3{al.x, al.y, al.z}, nullptr);
        }
    }
    row_ptr_w<uint2>(target, y)[x] = pack_h4(c);
}

}  // namespace
}  // namespace soc

using namespace soc;

namespace {
// The pair kernel of a form, per parameter-block type: each instantiation is named here once, with the form it is
// looked up by taken from the same template arguments. The plain forms: every pair of (hist, lights), the knobs' nt = 3
// and 7 without lights, and under the histogram the in-kernel bloom and the zero cells; the cascaded forms: (hist,
// lights); the bounded forms: the four lb of the stand-alone calls with and without the histogram, and bounded / cull
// under the histogram's bl and sp.
template <class P> using PairKernel = void (*)(DImg, DImg, DImg, DImg, DImg, DImg, DImg, DImg, P, DImg, DImg);
template <class P> struct PairEntry {
    PairForm form;
    PairKernel<P> kernel;
};
template <bool HIST, bool LIGHTS, int NT = 0, bool BL = false, bool SP = false, int LB = 0, bool CS = false>
PairEntry<std::conditional_t<CS, CompParamsCascaded, std::conditional_t<LB != 0, CompParamsBounded, CompParams>>> pair_entry() {
    return {PairForm{HIST, LIGHTS, NT, BL, SP, LB, CS}, composition_pair<HIST, LIGHTS, NT, BL, SP, LB, CS>};
}
constexpr int kCull = kLbBounded | kLbCull, kCount = kLbBounded | kLbCount, kCullCount = kLbBounded | kLbCull | kLbCount;
const PairEntry<CompParams> kPlainPairs[] = {
    pair_entry<false, false>(), pair_entry<false, true>(), pair_entry<true, false>(), pair_entry<true, true>(),
    pair_entry<false, false, 3>(), pair_entry<false, false, 7>(), pair_entry<true, false, 3>(), pair_entry<true, false, 7>(),
    pair_entry<true, false, 7, true>(), pair_entry<true, false, 7, true, true>(),
    pair_entry<true, true, 0, true>(), pair_entry<true, true, 0, true, true>(), pair_entry<true, true, 0, false, true>()};
const PairEntry<CompParamsCascaded> kCascadedPairs[] = {
    pair_entry<false, false, 7, false, false, 0, true>(), pair_entry<false, true, 0, false, false, 0, true>(),
    pair_entry<true, false, 7, false, false, 0, true>(), pair_entry<true, true, 0, false, false, 0, true>()};
const PairEntry<CompParamsBounded> kBoundedPairs[] = {
    pair_entry<false, true, 0, false, false, kLbBounded>(), pair_entry<false, true, 0, false, false, kCull>(),
    pair_entry<false, true, 0, false, false, kCount>(), pair_entry<false, true, 0, false, false, kCullCount>(),
    pair_entry<true, true, 0, false, false, kLbBounded>(), pair_entry<true, true, 0, false, false, kCull>(),
    pair_entry<true, true, 0, false, false, kCount>(), pair_entry<true, true, 0, false, false, kCullCount>(),
    pair_entry<true, true, 0, true, false, kLbBounded>(), pair_entry<true, true, 0, true, false, kCull>(),
    pair_entry<true, true, 0, false, true, kLbBounded>(), pair_entry<true, true, 0, false, true, kCull>(),
    pair_entry<true, true, 0, true, true, kLbBounded>(), pair_entry<true, true, 0, true, true, kCull>()};

template <class P, size_t N>
PairKernel<P> pair_kernel(const PairEntry<P> (&table)[N], const PairForm& f) {
    for (const PairEntry<P>& e : table) {
        const PairForm& t = e.form;
        if (t.hist == f.hist && t.lights == f.lights && t.nt == f.nt && t.bl == f.bl && t.sp == f.sp && t.lb == f.lb && t.cs == f.cs)
            return e.kernel;
    }
    return nullptr;   // a form no kernel exists for
}

// Launches what plan_composition decided: the kernel, then the fold of the 8 partial histograms.
int issue_composition(const CompositionPlan& pl, soc_stream stream) {
    const dim3 grd(pl.grid_x, pl.grid_y), blk(pl.block_x, pl.block_y);
    auto go = [&](const char* name, auto kernel, const auto&... tail) {
        if (!kernel) return set_error(SOC_E_INVALID_ARG, "soc_composition: no %s of the planned form", name);
        const DImg* im = pl.img;
        launch(name, kWorkgroup, kernel, grd, blk, 0, hs(stream), im[0], im[1], im[2], im[3], im[4], im[5], im[6], im[7], tail...);
        return (int)SOC_OK;
    };
    const CompParams& p = pl.p;
    int rc;
    if (pl.kernel == kCompGeneric) {
        rc = go("composition_generic", composition_generic, p);
    } else if (pl.kernel == kCompGenericBounded) {
        rc = go("composition_generic_bounded", composition_generic_bounded, p, pl.la.lb);
    } else if (pl.kernel == kCompGenericCascaded) {
        rc = go("composition_generic_cascaded", composition_generic_cascaded, pl.p);
    } else if (pl.form.cs) {
        rc = go("composition_pair", pair_kernel(kCascadedPairs, pl.form), pl.p, pl.mip1, pl.mip3);
    } else if (pl.form.lb) {
        CompParamsBounded pb;
        static_cast<CompParams&>(pb) = p;
        pb.la = pl.la;
        rc = go("composition_pair", pair_kernel(kBoundedPairs, pl.form), pb, pl.mip1, pl.mip3);
    } else {
        rc = go("composition_pair", pair_kernel(kPlainPairs, pl.form), p, pl.mip1, pl.mip3);
    }
    if (rc) return rc;
    if (pl.fold) launch("histogram_fold", kBins, histogram_fold, 1, kBins, 0, hs(stream), pl.scratch, pl.bins);
    return check_launch("composition");
}

}  // namespace

int soc::composition(const CompositionCall& c, soc_stream stream) {
    CompositionPlan pl;
    int rc = plan_composition(c, pl);
    if (!rc) rc = issue_composition(pl, stream);
    // not fusable: the two passes back to back (same results)
    if (!rc && pl.histogram_pass) rc = soc_generate_luminance_histogram(c.g, c.target, c.ae, stream);
    return rc;
}

int soc::sky_compose_launch(const soc_globals* g, soc_img target, soc_img depth, soc_img clouds, uint32_t* scratch,
                            soc_stream stream) {
    SkyComposePlan pl;
    const int rc = plan_sky_compose(g, target, depth, clouds, scratch, pl);
    if (rc) return rc;
    launch("sky_compose_pair", kWorkgroup, pl.pair_load ? sky_compose_pair<true> : sky_compose_pair<false>,
           dim3(pl.grid_x, pl.grid_y), kWorkgroup, 0, hs(stream), pl.target, pl.depth, pl.clouds, pl.p);
    return check_launch("sky_compose");
}

int soc::histogram_fold_launch(uint32_t* scratch, soc_auto_exposure* ae, soc_stream stream) {
    if (!scratch || !ae) return set_error(SOC_E_INVALID_ARG, "histogram fold: null scratch / auto exposure");
    launch("histogram_fold", kBins, histogram_fold, 1, kBins, 0, hs(stream), scratch, ae->histogram_buckets);
    return check_launch("luminance_histogram_fold");
}

extern "C" int soc_composition(const soc_globals* g, const soc_globals* d_globals, soc_img target, soc_img albedo,
                               soc_img emissive, soc_img normal, soc_img depth, soc_img ssao, soc_img shadow,
                               soc_img clouds, soc_stream stream) {
    return composition(composition_call(g, d_globals, {target, albedo, emissive, normal, depth, ssao, shadow, clouds}), stream);
}

extern "C" int soc_composition_bounded(const soc_globals* g, const soc_globals* d_globals, soc_img target, soc_img albedo,
                                       soc_img emissive, soc_img normal, soc_img depth, soc_img ssao, soc_img shadow,
                                       soc_img clouds, const void* d_bounds, uint32_t flags, uint32_t* d_shaded_pairs,
                                       soc_stream stream) {
    const LightBoundsCall bc = {d_bounds, flags, d_shaded_pairs};
    CompositionCall c = composition_call(g, d_globals, {target, albedo, emissive, normal, depth, ssao, shadow, clouds});
    c.bounds = &bc;
    return composition(c, stream);
}

extern "C" int soc_composition_cascaded(const soc_globals* g, const soc_globals* d_globals, soc_img target, soc_img albedo,
                                        soc_img emissive, soc_img normal, soc_img depth, soc_img ssao, soc_img shadow,
                                        soc_img clouds, const soc_sun_cascades* cascades, soc_stream stream) {
    CompositionCall c = composition_call(g, d_globals, {target, albedo, emissive, normal, depth, ssao, shadow, clouds});
    c.cascades = cascades;
    c.cascaded = true;
    return composition(c, stream);
}

extern "C" int soc_composition_luminance_histogram(const soc_globals* g, const soc_globals* d_globals, soc_img target,
                                                   soc_img albedo, soc_img emissive, soc_img normal, soc_img depth,
                                                   soc_img ssao, soc_img shadow, soc_img clouds, soc_auto_exposure* ae,
                                                   uint32_t* scratch, soc_stream stream) {
    CompositionCall c = composition_call(g, d_globals, {target, albedo, emissive, normal, depth, ssao, shadow, clouds});
    c.histogram = c.fold = true;
    c.ae = ae;
    c.scratch = scratch;
    return composition(c, stream);
}

extern "C" int soc_composition_luminance_histogram_bounded(const soc_globals* g, const soc_globals* d_globals, soc_img target,
                                                           soc_img albedo, soc_img emissive, soc_img normal, soc_img depth,
                                                           soc_img ssao, soc_img shadow, soc_img clouds, soc_auto_exposure* ae,
                                                           uint32_t* scratch, const void* d_bounds, uint32_t flags,
                                                           uint32_t* d_shaded_pairs, soc_stream stream) {
    const LightBoundsCall bc = {d_bounds, flags, d_shaded_pairs};
    CompositionCall c = composition_call(g, d_globals, {target, albedo, emissive, normal, depth, ssao, shadow, clouds});
    c.histogram = c.fold = true;
    c.ae = ae;
    c.scratch = scratch;
    c.bounds = &bc;
    return composition(c, stream);
}

extern "C" int soc_composition_luminance_histogram_cascaded(const soc_globals* g, const soc_globals* d_globals, soc_img target,
                                                            soc_img albedo, soc_img emissive, soc_img normal, soc_img depth,
                                                            soc_img ssao, soc_img shadow, soc_img clouds, soc_auto_exposure* ae,
                                                            uint32_t* scratch, const soc_sun_cascades* cascades,
                                                            soc_stream stream) {
    if (!cascades) return set_error(SOC_E_INVALID_ARG, "soc_composition_luminance_histogram_cascaded: null cascades");
    CompositionCall c = composition_call(g, d_globals, {target, albedo, emissive, normal, depth, ssao, shadow, clouds});
    c.histogram = c.fold = true;
    c.ae = ae;
    c.scratch = scratch;
    c.cascades = cascades;
    c.cascaded = true;
    return composition(c, stream);
}
