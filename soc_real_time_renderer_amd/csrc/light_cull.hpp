// light_cull.hpp — the two wave-level culling predicates of Composition's bounded lights (composition.hip, CULL), as
// plain inline functions with no HIP in them: the kernel calls them per (wave patch, light), tools/check_light_cull.cpp
// calls the same text on the host against float64 geometry (tests/test_light_cull.py).
//
// A predicate answers "cull" only when no pixel of the patch can pass the PER-PIXEL test as the device computes it, so
// a culled light and the same light evaluated and rejected pixel by pixel leave the same bits. Each has a stated slack
// and culls at TWICE that slack in its own float arithmetic; the guarantee handed out (and checked in float64 by the
// tool) is the single slack, which in turn exceeds what the per-pixel side can lose. u = 2^-24 (half an fp32 ulp,
// relative). Neither slack was fitted to a test result.
//
// Range (kRangeSlack = 2^-18 = 64 u). Per pixel the window is positive iff q < 1 with q = fl(d2 * inv_r2), d2 the
// kernel's fma chain dot(l, l), l = fl(light - pos), inv_r2 = fl(1 / fl(r * r)) from the upload:
//   l's components carry (1 + u) each, their squares (1 + u)^2, and the chain of three non-negative terms at most
//   three more roundings: d2 >= d2_exact * (1 - 5u);   inv_r2 >= (1 / r2)(1 - u), r2 = fl(r * r) the stored square;
//   the product one more: q >= (d2_exact / r2)(1 - 7u).  v_rsq_f32 takes no part in q.
// So a pixel with d2_exact >= r2 (1 + 8u) is rejected per pixel. The predicate's own distance to the box, D2, is three
// differences (1 + u), squares and a sum of non-negative terms like the above: D2_exact >= D2 (1 - 5u), and every
// pixel in the box has d2_exact >= D2_exact. Culling at D2 >= r2 (1 + 2 * 64u) gives d2_exact >= r2 (1 + 128u)(1 - 5u)
// >= r2 (1 + 64u): the stated slack, eight times the 8u needed. (r2 and D2 are assumed normal numbers: a range
// below 1e-18 is not a light.)
//
// Cone (kConeSlack = 2^-16 = 256 u, absolute on a cosine). Per pixel the cone term is positive only if theta > outer
// (cut_off > outer_cut_off, else the predicate does not cull), theta = dot(ld, sd) * sk with ld = l * rsq(d2),
// sk = rsq(|sd|^2): v_rsq_f32 is good to 1 ulp = 2u, so each ld component carries (1 + u)(d2's 5u / 2)(2u)(1 + u) <= 7u,
// the products and the chain 3u more, sk 2u + 3u and its product u: |theta - cos(angle)| <= 16u |ld||sd| sk <= 17u by
// Cauchy-Schwarz. A pixel with cos_exact <= outer - 17u is rejected. The predicate bounds cos over the box's bounding
// sphere (centre C, radius R, apex A, unit axis a, v = C - A, dist = |v|): every point P of the sphere has
// angle(P - A, a) >= alpha - beta, alpha the angle of v to the axis, beta = asin(R / dist) the sphere's angular radius,
// provided dist > R and alpha >= beta; then max cos = cos(alpha - beta) = cos a cos b + sin a sin b, also right for a
// sphere behind the apex (alpha up to pi) and for outer < 0. In fp32: cos a = dot(v, a) / dist (<= 8u absolute),
// sin a = |v x a| / dist from the cross product, which has no cancellation near alpha = 0 or pi (<= 8u),
// sin b = sqrt(R^2 / dist^2) (<= 4u), cos b = sqrt(y), y = (dist^2 - R^2) / dist^2 (<= 8u absolute in y, hence
// <= 8u / (2 sqrt(y)) <= 32u in cos b once y >= 1/64; a sphere closer to the apex than that is not culled), two
// products and a sum: <= 60u in all. The sphere itself is rounded outwards (centre error <= u |C_i| per axis, radius
// (1 + 3u)): R is taken as R (1 + 2^-20) + 2^-22 (|Cx| + |Cy| + |Cz|). Culling at cos(alpha - beta) <= outer - 2 * 256u
// gives cos_exact <= outer - 512u + 60u <= outer - 256u: the stated slack, fifteen times the 17u needed.
//
// Non-finite input (an infinite box from an Inf position, a NaN axis from a zero direction) makes a comparison false
// and the answer "keep".
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SOC_LC_FN __host__ __device__ inline
#else
#define SOC_LC_FN inline
#endif

namespace soc {
namespace light_cull {

constexpr float kRangeSlack = 1.0f / 262144.0f;   // 2^-18, relative on d^2 / r^2
constexpr float kConeSlack = 1.0f / 65536.0f;     // 2^-16, absolute on cos(theta)

struct Aabb {   // scalar members, no indexed arrays: the device keeps a box in registers
    float lox, loy, loz, hix, hiy, hiz;
};

SOC_LC_FN float lc_max(float a, float b) { return a > b ? a : b; }
SOC_LC_FN float lc_abs(float a) { return a < 0.0f ? -a : a; }
SOC_LC_FN float lc_sqrt(float a) { return __builtin_sqrtf(a); }   // correctly rounded on the host and on the device

// True: no point of the box is within the range whose square is r2 (> 0), with kRangeSlack to spare.
SOC_LC_FN bool sphere_outside_aabb(const Aabb& b, const float c[3], float r2) {
    const float ex = lc_max(lc_max(b.lox - c[0], c[0] - b.hix), 0.0f);
    const float ey = lc_max(lc_max(b.loy - c[1], c[1] - b.hiy), 0.0f);
    const float ez = lc_max(lc_max(b.loz - c[2], c[2] - b.hiz), 0.0f);
    const float d2 = ex * ex + ey * ey + ez * ez;
    return d2 >= r2 * (1.0f + 2.0f * kRangeSlack);
}

// True: no point of the box's bounding sphere has cos(angle to the axis `dir` from `apex`) > outer - kConeSlack.
// `dir` need not be unit (the kernel normalises the record's direction the same way); cut_off <= outer: never culls.
SOC_LC_FN bool cone_outside_aabb(const Aabb& b, const float apex[3], const float dir[3], float cut_off, float outer) {
    if (!(cut_off > outer)) return false;
    const float c0 = 0.5f * (b.lox + b.hix), c1 = 0.5f * (b.loy + b.hiy), c2 = 0.5f * (b.loz + b.hiz);
    const float e0 = b.hix - b.lox, e1 = b.hiy - b.loy, e2 = b.hiz - b.loz;
    const float vx = c0 - apex[0], vy = c1 - apex[1], vz = c2 - apex[2];
    const float ext2 = e0 * e0 + e1 * e1 + e2 * e2;
    const float cabs = lc_abs(c0) + lc_abs(c1) + lc_abs(c2);
    const float R = 0.5f * lc_sqrt(ext2) * (1.0f + 1.0f / 1048576.0f) + cabs * (1.0f / 4194304.0f);
    const float R2 = R * R;
    const float dist2 = vx * vx + vy * vy + vz * vz;
    const float a2 = dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2];
    if (!(dist2 > R2) || !(a2 > 0.0f)) return false;
    const float y = (dist2 - R2) / dist2;            // cos^2 of the sphere's angular radius
    if (!(y >= 1.0f / 64.0f)) return false;
    const float inv = 1.0f / lc_sqrt(dist2 * a2);
    const float cos_a = (vx * dir[0] + vy * dir[1] + vz * dir[2]) * inv;
    const float cx = vy * dir[2] - vz * dir[1], cy = vz * dir[0] - vx * dir[2], cz = vx * dir[1] - vy * dir[0];
    const float sin_a = lc_sqrt(cx * cx + cy * cy + cz * cz) * inv;
    const float cos_b = lc_sqrt(y), sin_b = lc_sqrt(R2 / dist2);
    if (!(cos_a <= cos_b)) return false;             // the axis passes through the sphere
    return cos_a * cos_b + sin_a * sin_b <= outer - 2.0f * kConeSlack;
}

}  // namespace light_cull
}  // namespace soc
