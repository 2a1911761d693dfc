// check_light_cull — the culling predicates of csrc/light_cull.hpp against float64 geometry (tests/test_light_cull.py).
//
// Draws seeded (box, light) cases. Whenever a predicate answers "cull", every one of 68 sampled points of the box (its
// 8 corners, 12 edge midpoints, 6 face centres, the centre, the point nearest the light and 40 random points) must
// satisfy, in float64, d^2 >= r^2 (1 + kRangeSlack) respectively cos(theta) <= outer_cut_off - kConeSlack: the
// guarantee the header states. A fixed share of the cases grazes a boundary: the range sphere or the cone surface
// passes within 1e-4 (relative) of a corner, an edge or a face of the box, on either side; the apex lies inside the box
// or the box lies behind it. Lights placed far away (by a wide margin in float64) must in fact be culled.
//   g++ -O2 tools/check_light_cull.cpp -o check_light_cull && ./check_light_cull [cases]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../soc_real_time_renderer_amd/csrc/light_cull.hpp"

using soc::light_cull::Aabb;

namespace {
uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t next_u64() {   // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
double uni() { return (double)(next_u64() >> 11) * (1.0 / 9007199254740992.0); }
double uni(double a, double b) { return a + (b - a) * uni(); }
int pick(int n) { return (int)(next_u64() % (uint64_t)n); }

struct V {
    double x, y, z;
};
V operator+(V a, V b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
V operator-(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V operator*(V a, double s) { return {a.x * s, a.y * s, a.z * s}; }
double dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
V cross(V a, V b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double len(V a) { return std::sqrt(dot(a, a)); }
V unit(V a) { return a * (1.0 / len(a)); }
V random_unit() {
    for (;;) {
        V v = {uni(-1, 1), uni(-1, 1), uni(-1, 1)};
        const double l = len(v);
        if (l > 0.1 && l <= 1.0) return v * (1.0 / l);
    }
}
double comp(const V& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : v.z; }
void set(V& v, int k, double s) { (k == 0 ? v.x : k == 1 ? v.y : v.z) = s; }

// the box as the kernel has it: float corners
struct Box {
    Aabb f;
    V lo, hi;
};
Box random_box() {
    Box b;
    const double scale = std::exp(uni(std::log(0.01), std::log(20.0)));
    V c = {uni(-50, 50), uni(-50, 50), uni(-50, 50)};
    V h = {scale * uni(0.0, 1.0), scale * uni(0.0, 1.0), scale * uni(0.0, 1.0)};
    if (pick(8) == 0) h.x = 0.0;   // a degenerate axis (a wave patch on a wall)
    b.f = Aabb{(float)(c.x - h.x), (float)(c.y - h.y), (float)(c.z - h.z), (float)(c.x + h.x), (float)(c.y + h.y), (float)(c.z + h.z)};
    b.lo = {b.f.lox, b.f.loy, b.f.loz};
    b.hi = {b.f.hix, b.f.hiy, b.f.hiz};
    return b;
}
// a point of the box's surface on a corner (3 clamped axes), an edge (2) or a face (1), and an outward direction
// whose nearest box point it is
void surface_point(const Box& b, int clamped, V& p, V& out) {
    int order[3] = {0, 1, 2};
    for (int i = 2; i > 0; --i) {
        const int j = pick(i + 1), t = order[i];
        order[i] = order[j];
        order[j] = t;
    }
    out = {0, 0, 0};
    for (int i = 0; i < 3; ++i) {
        const int k = order[i];
        if (i < clamped) {
            const bool high = pick(2) != 0;
            set(p, k, high ? comp(b.hi, k) : comp(b.lo, k));
            set(out, k, (high ? 1.0 : -1.0) * uni(0.05, 1.0));
        } else {
            set(p, k, uni(comp(b.lo, k), comp(b.hi, k)));
        }
    }
    out = unit(out);
}

constexpr int kSamples = 68;
void samples(const Box& b, V light, V* s) {
    int n = 0;
    for (int i = 0; i < 27; ++i) {   // corners, edge midpoints, face centres, centre
        const int t[3] = {i % 3, (i / 3) % 3, i / 9};
        V p;
        for (int k = 0; k < 3; ++k) set(p, k, t[k] == 0 ? comp(b.lo, k) : t[k] == 1 ? comp(b.hi, k) : 0.5 * (comp(b.lo, k) + comp(b.hi, k)));
        s[n++] = p;
    }
    V near;
    for (int k = 0; k < 3; ++k) set(near, k, std::fmin(std::fmax(comp(light, k), comp(b.lo, k)), comp(b.hi, k)));
    s[n++] = near;
    while (n < kSamples) {
        V p;
        for (int k = 0; k < 3; ++k) {
            const int w = pick(4);   // on a face of this axis half of the time
            set(p, k, w == 0 ? comp(b.lo, k) : w == 1 ? comp(b.hi, k) : uni(comp(b.lo, k), comp(b.hi, k)));
        }
        s[n++] = p;
    }
}
}  // namespace

int main(int argc, char** argv) {
    const long cases = argc > 1 ? std::atol(argv[1]) : 1200000;
    const double dr = soc::light_cull::kRangeSlack, dc = soc::light_cull::kConeSlack;
    long failures = 0, range_culled = 0, cone_culled = 0, grazing = 0, far_range = 0, far_cone = 0, apex_inside = 0, behind = 0;
    V smp[kSamples];
    for (long c = 0; c < cases; ++c) {
        const Box b = random_box();
        const V centre = (b.lo + b.hi) * 0.5;
        const double R = 0.5 * len(b.hi - b.lo);
        const int mode = (int)(c % 8);   // 0, 1: grazing; 2: far; 3: apex inside / box behind; else random
        // ---- range
        {
            V light;
            double r;
            bool far = false;
            if (mode < 2) {
                V p, out;
                surface_point(b, 1 + pick(3), p, out);
                const double dist = std::exp(uni(std::log(0.05), std::log(30.0)));
                light = p + out * dist;
                r = dist * (1.0 + uni(-1e-4, 1e-4));
                ++grazing;
            } else if (mode == 2) {
                r = std::exp(uni(std::log(0.05), std::log(30.0)));
                light = centre + random_unit() * (3.0 * (r + R) + 1.0);
                far = true;
                ++far_range;
            } else {
                r = std::exp(uni(std::log(0.05), std::log(60.0)));
                light = centre + random_unit() * uni(0.0, 2.0 * (r + R));
            }
            const float lf[3] = {(float)light.x, (float)light.y, (float)light.z};
            const float r2 = (float)r * (float)r;
            const bool cull = soc::light_cull::sphere_outside_aabb(b.f, lf, r2);
            const V l64 = {lf[0], lf[1], lf[2]};
            if (far && !cull) {
                if (++failures <= 10) std::printf("range: far light not culled (case %ld)\n", c);
            }
            if (cull) {
                ++range_culled;
                samples(b, l64, smp);
                for (int i = 0; i < kSamples; ++i) {
                    const V d = smp[i] - l64;
                    if (!(dot(d, d) >= (double)r2 * (1.0 + dr))) {
                        if (++failures <= 10) std::printf("range: culled, but d2 / r2 = %.9f at sample %d (case %ld)\n", dot(d, d) / r2, i, c);
                        break;
                    }
                }
            }
        }
        // ---- cone
        {
            const double phi = uni(0.05, 2.6);           // outer half-angle, up to beyond a hemisphere
            const double outer = std::cos(phi), cut = std::cos(phi * uni(0.3, 0.95));
            V apex, axis;
            bool far = false;
            if (mode < 2) {   // the cone's surface passes within 1e-4 of a corner, an edge or a face point
                V p, out;
                surface_point(b, 1 + pick(3), p, out);
                apex = p + random_unit() * std::exp(uni(std::log(0.05), std::log(30.0)));
                const V to = unit(p - apex);
                V perp = cross(to, random_unit());
                if (len(perp) < 1e-3) perp = cross(to, V{1, 0, 0});
                perp = unit(perp);
                const double a = phi * (1.0 + uni(-1e-4, 1e-4));
                axis = to * std::cos(a) + perp * std::sin(a);
            } else if (mode == 2) {   // the box well outside the cone: by 0.3 rad beyond its angular radius
                const double dist = R * uni(2.0, 30.0) + 0.1;
                const double beta = std::asin(std::fmin(1.0, R / dist));
                const double alpha = phi + beta + 0.3;
                if (alpha < 3.1) {
                    const V to = random_unit();
                    V perp = cross(to, random_unit());
                    if (len(perp) < 1e-3) perp = cross(to, V{1, 0, 0});
                    perp = unit(perp);
                    apex = centre - to * dist;
                    axis = to * std::cos(alpha) + perp * std::sin(alpha);
                    far = true;
                    ++far_cone;
                } else {
                    apex = centre - random_unit() * dist;
                    axis = random_unit();
                }
            } else if (mode == 3) {
                if (pick(2)) {   // the apex inside the box
                    apex = {uni(b.lo.x, b.hi.x), uni(b.lo.y, b.hi.y), uni(b.lo.z, b.hi.z)};
                    axis = random_unit();
                    ++apex_inside;
                } else {         // the box behind the apex, the axis pointing away from it (nearly)
                    apex = centre + random_unit() * (R * uni(1.0, 4.0) + 0.01);
                    axis = unit(unit(apex - centre) + random_unit() * uni(0.0, 0.5));
                    ++behind;
                }
            } else {
                apex = centre + random_unit() * uni(0.0, 4.0 * R + 5.0);
                axis = random_unit();
            }
            axis = axis * uni(0.2, 3.0);   // the record's direction is not unit
            const float af[3] = {(float)apex.x, (float)apex.y, (float)apex.z};
            const float df[3] = {(float)axis.x, (float)axis.y, (float)axis.z};
            const float cutf = (float)cut, outerf = (float)outer;
            const bool cull = soc::light_cull::cone_outside_aabb(b.f, af, df, cutf, outerf);
            if (far && cutf > outerf && !cull) {
                if (++failures <= 10) std::printf("cone: far box not culled (case %ld)\n", c);
            }
            if (cull) {
                ++cone_culled;
                const V a64 = {af[0], af[1], af[2]}, d64 = {df[0], df[1], df[2]};
                samples(b, a64, smp);
                for (int i = 0; i < kSamples; ++i) {
                    const V d = smp[i] - a64;
                    const double l = len(d);
                    if (l == 0.0) continue;
                    const double ct = dot(d, d64) / (l * len(d64));
                    if (!(ct <= (double)outerf - dc)) {
                        if (++failures <= 10) std::printf("cone: culled, but cos = %.9f > outer %.9f - slack at sample %d (case %ld)\n", ct, (double)outerf, i, c);
                        break;
                    }
                }
            }
        }
    }
    std::printf("cases %ld: grazing %ld, far range %ld, far cone %ld, apex inside %ld, box behind %ld; range culled %ld, cone culled %ld; failures %ld\n",
                cases, grazing, far_range, far_cone, apex_inside, behind, range_culled, cone_culled, failures);
    return failures ? 1 : 0;
}
