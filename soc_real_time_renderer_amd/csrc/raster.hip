// raster.hip — depth prepass / G-buffer / sun-shadow rasterisation for gfx950.
//
// Replaces the reference's fixed-function raster producers upstream of the screen-space chain:
//   DepthPrepassTask      depth_prepass.inl:26-120      (cull FRONT, LESS_OR_EQUAL)
//   GBufferGenerationTask g_buffer_generation.inl:33-230 (cull FRONT, LESS_OR_EQUAL, depth LOAD)
//   SunShadowDrawTask     sun_shadow_draw.inl:27-91     (cull BACK, depth bias 1.25 / 1.75)
// gfx950 has no raster units reachable from HIP, so the raster is a compute visibility buffer:
//   1. raster_setup     one lane per vertex: object -> world -> clip -> screen (x, y, z_ndc, 1/w)
//   2. raster_small     one lane per triangle: cull, bounding box; a box of <= SMALL_PIXELS pixels is
//                       scanned by the lane itself, larger ones are split into 32x32-pixel tiles
//   3. raster_big       one wave per (triangle, tile) work item: tiles that an edge function excludes at
//                       all four corners (with a rounding margin) are skipped, else 64 lanes cover the
//                       tile's 1024 pixels
//   every covered pixel does ONE 64-bit atomicMin of (depth bits << 32 | 0xFFFFFFFE - triangle): with
//   z >= 0 the float bits order like the depths, and ties keep the LATER triangle, which is exactly the
//   serial LESS_OR_EQUAL result in draw order. The depth-only variant (shadow map) does a 32-bit
//   atomicMin of the biased depth bits straight into the D32 image.
//   4. gbuffer_resolve  one lane per pixel: the winning triangle's perspective-correct barycentrics,
//                       attribute interpolation and the GBufferGeneration fragment shader
//                       (g_buffer_generation.inl:189-225).
// The coverage, depth and barycentric arithmetic is written without FMA contraction and matches the
// oracle's (oracle/soc_oracle.c, soc_oracle_raster_*) operation for operation, so the visibility buffer
// and the depth images are bit-exact against it.
// A scene of per-entity draws with their own transforms (soc_draw_scene) runs the same triangle and pixel kernels on
// tables built at load time, behind draw-aware versions of the two vertex kernels: see "Draw scenes" below.
// The terrain tasks that draw over the entity tasks' images (DrawTerrainTask draw_terrain.inl, SunShadowDrawTerrainTask
// sun_shadow_draw_terrain.inl: depth LOAD, LESS_OR_EQUAL) are a layer: the same raster kernels into a visibility buffer of
// the layer's own (or, depth-only, into the shadow image without the clear), then the resolve's LAYER form, which
// depth-tests each pixel against the image that is there: see "Terrain layer" below.
// This file holds every raster kernel and the entry points that issue them; the resolve's texture sampler is
// raster_sampler.hpp, and what the entry points check and lay out before any HIP call is raster_host.cpp.
#include <vector>

#include "luminance.hpp"
#include "raster_host.hpp"
#include "raster_sampler.hpp"
#include "soc_internal.hpp"

namespace soc {
namespace {

constexpr int SMALL_PIXELS = 64;    // bounding boxes up to this many pixels are scanned by one lane
#ifndef SOC_RASTER_TILE
#define SOC_RASTER_TILE 32
#endif
constexpr int TILE = SOC_RASTER_TILE;   // large-triangle work item: a TILE x TILE tile of its bounding box
#ifndef SOC_RASTER_FIXED_COLS
#define SOC_RASTER_FIXED_COLS 0   // A/B builds: raster_big's lanes as 32 x 2 pixels whatever the item's width
#endif
static_assert(TILE == 32 || SOC_RASTER_FIXED_COLS, "raster_big's lane layout covers items up to 32 pixels wide");
constexpr uint32_t KEY_EMPTY = 0xFFFFFFFFu;

struct RasterParams {
    Mat4 model, vp;
    int width, height, vertex_count, triangle_count;
    int cull;
    int depth_only;
    float bias_constant, bias_slope;
    int small_pixels;   // boxes up to this many pixels are scanned by one lane
};

// The raster workspace (raster_layout, raster_host.hpp) as pointers.
// The counter packs (large triangles << 40 | tiles so far): one 64-bit atomicAdd per large triangle
// returns its entry slot and the first index of its tile range together, so the entries are in
// increasing range order and a work index finds its triangle by binary search.
struct Workspace {
    float4* screen;
    unsigned long long* counter;
    uint2* entries;   // {triangle, first tile index (low 32 bits of the range start)}
    float4* vdata;    // G-buffer resolve: 4 float4 per vertex (gbuffer_vertex_setup)
};
constexpr int ENTRY_SHIFT = 40;

inline Workspace carve(void* ws, int V, int T) {
    char* p = static_cast<char*>(ws);
    const RasterLayout l = raster_layout(V, T);
    return Workspace{reinterpret_cast<float4*>(p), reinterpret_cast<unsigned long long*>(p + l.counter),
                     reinterpret_cast<uint2*>(p + l.entries), reinterpret_cast<float4*>(p + l.vdata)};
}

// GLSL mat4 * vec4, summed left to right, no contraction (the oracle's mat_vec).
__device__ __forceinline__ f4 mat_vec_exact(const Mat4& M, float x, float y, float z, float w) {
#pragma clang fp contract(off)
    const float* m = M.m;
    return f4{m[0] * x + m[4] * y + m[8] * z + m[12] * w, m[1] * x + m[5] * y + m[9] * z + m[13] * w,
              m[2] * x + m[6] * y + m[10] * z + m[14] * w, m[3] * x + m[7] * y + m[11] * z + m[15] * w};
}

// Homogeneous screen-space vertex (2DH rasterisation, Olano & Greer): X = (x_c/2 + w_c/2) W,
// Y = (y_c/2 + w_c/2) H (y = 0 top row, uv = ndc * 0.5 + 0.5), Z = z_c, W = w_c. No division, so
// vertices behind the eye need no geometric clipping; fragments with z_ndc outside [0, 1] are clipped
// per pixel (Vulkan depth clipping; the reference's RH_NO projection puts z_c = 0 between near and far).
__device__ __forceinline__ float4 clip_vertex(const float* __restrict__ pos, int v, const Mat4& model, const Mat4& vp,
                                              int W, int H) {
#pragma clang fp contract(off)
    const float px = pos[3 * v], py = pos[3 * v + 1], pz = pos[3 * v + 2];
    const f4 wp = mat_vec_exact(model, px, py, pz, 1.0f);
    const f4 c = mat_vec_exact(vp, wp.x, wp.y, wp.z, wp.w);
    return float4{(c.x * 0.5f + c.w * 0.5f) * (float)W, (c.y * 0.5f + c.w * 0.5f) * (float)H, c.z, c.w};
}

__device__ __forceinline__ f3 cross_exact(f3 a, f3 b) {
#pragma clang fp contract(off)
    return f3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

struct TriSetup {
    f3 r0, r1, r2;          // edge functions E_i(p) = r_i . (px, py, 1), sign-normalised: inside iff all >= 0
    float z0, z1, z2, w0, w1, w2;
    float bias;
    int px0, px1, py0, py1;
    bool live;
};

// Screen bounding box of the part of a triangle in front of the depth-clip plane z_c = 0: its vertices there and its
// edges' crossings of the plane, projected (wide: a point at w <= 1e-20, the box is the whole image). Plain values and
// flags in a struct (a capturing lambda here had its two flags spilled to scratch).
struct BBox {
    float minx = 3.0e38f, maxx = -3.0e38f, miny = 3.0e38f, maxy = -3.0e38f;
    bool any = false, wide = false;
};
__device__ __forceinline__ void bbox_add(BBox& b, float X, float Y, float Wc) {
#pragma clang fp contract(off)
    if (!(Wc > 1e-20f)) {
        b.wide = true;
        return;
    }
    const float x = X / Wc, y = Y / Wc;
    b.minx = fminf(b.minx, x); b.maxx = fmaxf(b.maxx, x);
    b.miny = fminf(b.miny, y); b.maxy = fmaxf(b.maxy, y);
    b.any = true;
}
// vertex a, and where the edge a -> b crosses z_c = 0
__device__ __forceinline__ void bbox_edge(BBox& bb, float4 a, float4 b) {
#pragma clang fp contract(off)
    if (a.z >= 0.0f) bbox_add(bb, a.x, a.y, a.w);
    if ((a.z >= 0.0f) != (b.z >= 0.0f)) {
        const float u = a.z / (a.z - b.z);
        bbox_add(bb, a.x + u * (b.x - a.x), a.y + u * (b.y - a.y), a.w + u * (b.w - a.w));
    }
}

// Triangle setup: the adjugate rows r_i of [v0 v1 v2] (v = (X, Y, W)), det = v0 . r0. Facing is the
// sign of det (= the sign of the framebuffer area when every w > 0; Vulkan a = -area/2 < 0 is
// clockwise = front, the reference pipelines' winding: see soc_rt.h). Bounding box from the projected vertices when every w > 1e-6, else the
// whole image. Depth bias: z_ndc = (sum z_i r_i) . p / |det| is affine in the pixel position.
__device__ __forceinline__ TriSetup tri_setup(float4 A, float4 B, float4 C, const RasterParams& p) {
#pragma clang fp contract(off)
    TriSetup t;
    t.live = false;
    // Wholly beyond the far plane: every vertex has w_c > 0 and z_c > w_c (1 + 2^-12). A covered pixel's E_i are >= 0, so
    // z_ndc = sum E_i z_i / sum E_i w_i sums non-negative terms, each fp32 rounding is relative (<= 7 of 2^-24 in all),
    // and the ratio is >= min z_i / w_i >= 1 + 2^-12: the computed z_ndc is > 1 and cover() clips every pixel. Skipping
    // the triangle writes the same (nothing). The sun's orthographic frustum leaves most of the mesh beyond its far plane.
    {
        constexpr float kFar = 1.0f + 1.0f / 4096.0f;
        if (A.w > 0.0f && B.w > 0.0f && C.w > 0.0f && A.z > A.w * kFar && B.z > B.w * kFar && C.z > C.w * kFar) return t;
    }
    const f3 v0{A.x, A.y, A.w}, v1{B.x, B.y, B.w}, v2{C.x, C.y, C.w};
    f3 r0 = cross_exact(v1, v2), r1 = cross_exact(v2, v0), r2 = cross_exact(v0, v1);
    const float det = v0.x * r0.x + v0.y * r0.y + v0.z * r0.z;
    if (!(det != 0.0f) || det != det) return t;
    if (p.cull == SOC_CULL_FRONT && det > 0.0f) return t;
    if (p.cull == SOC_CULL_BACK && det < 0.0f) return t;
    if (det < 0.0f) { r0 = -r0; r1 = -r1; r2 = -r2; }
    t.r0 = r0; t.r1 = r1; t.r2 = r2;
    t.z0 = A.z; t.z1 = B.z; t.z2 = C.z;
    t.w0 = A.w; t.w1 = B.w; t.w2 = C.w;
    // Bounding box of the triangle clipped to z_c >= 0 (fragments below it are depth-clipped anyway, and
    // there w > 0 for a perspective or orthographic projection), one pixel of margin: a superset of the
    // covered centres. The oracle scans the whole image for such triangles; coverage itself is decided
    // per pixel by the edge functions only, so the results are identical.
    {
        BBox bb;
        bbox_edge(bb, A, B);
        bbox_edge(bb, B, C);
        bbox_edge(bb, C, A);
        const float minx = bb.minx, maxx = bb.maxx, miny = bb.miny, maxy = bb.maxy;
        const bool any = bb.any, wide = bb.wide;
        if (!any && !wide) return t;   // wholly behind the depth-clip plane
        const float W = (float)p.width, H = (float)p.height;
        if (wide || minx != minx || miny != miny || maxx != maxx || maxy != maxy) {
            t.px0 = 0; t.px1 = p.width - 1; t.py0 = 0; t.py1 = p.height - 1;
        } else {
            t.px0 = max(0, (int)floorf(fminf(fmaxf(minx - 1.5f, -1.0f), W)));
            t.px1 = min(p.width - 1, (int)ceilf(fminf(fmaxf(maxx + 0.5f, -1.0f), W)));
            t.py0 = max(0, (int)floorf(fminf(fmaxf(miny - 1.5f, -1.0f), H)));
            t.py1 = min(p.height - 1, (int)ceilf(fminf(fmaxf(maxy + 0.5f, -1.0f), H)));
        }
    }
    if (t.px0 > t.px1 || t.py0 > t.py1) return t;
    t.bias = 0.0f;
    if (p.depth_only) {   // Vulkan depth bias: m * slope + r * constant
        const float adet = fabsf(det);
        const float nx = A.z * r0.x + B.z * r1.x + C.z * r2.x, ny = A.z * r0.y + B.z * r1.y + C.z * r2.y;
        const float m = fmaxf(fabsf(nx / adet), fabsf(ny / adet));
        // r = 2^(E - 23), E the exponent of the largest |z_ndc| at a vertex (in front of the eye)
        float zmax = 0.0f;
        if (A.w > 0.0f) zmax = fmaxf(zmax, fabsf(A.z / A.w));
        if (B.w > 0.0f) zmax = fmaxf(zmax, fabsf(B.z / B.w));
        if (C.w > 0.0f) zmax = fmaxf(zmax, fabsf(C.z / C.w));
        const uint32_t ebits = (__float_as_uint(zmax) >> 23) & 255u;
        const float r = (ebits == 0u || ebits == 255u) ? 0.0f : ldexpf(1.0f, (int)ebits - 127 - 23);
        t.bias = m * p.bias_slope + r * p.bias_constant;
    }
    t.live = true;
    return t;
}

// An edge owns the pixel centres exactly on it iff its normal (r.x, r.y) points to +x, or to +y when
// vertical: shared edges have exactly negated coefficients, so each such centre is covered once.
__device__ __forceinline__ bool owns(f3 r) { return r.x > 0.0f || (r.x == 0.0f && r.y > 0.0f); }

__device__ __forceinline__ float edge(f3 r, float px, float py) {
#pragma clang fp contract(off)
    return r.x * px + r.y * py + r.z;
}

// Coverage of pixel (x, y): the three edge functions at the pixel centre, the tie rule, then
// z_ndc = sum E_i z_i / sum E_i w_i and depth clipping. e0..e2 are returned for the barycentrics
// (perspective-correct b_i = E_i / sum E). z is +0 for a -0 result.
__device__ __forceinline__ bool cover(const TriSetup& t, int x, int y, float& e0, float& e1, float& e2, float& z) {
#pragma clang fp contract(off)
    const float fx = (float)x + 0.5f, fy = (float)y + 0.5f;
    e0 = edge(t.r0, fx, fy);
    e1 = edge(t.r1, fx, fy);
    e2 = edge(t.r2, fx, fy);
    if (e0 < 0.0f || e1 < 0.0f || e2 < 0.0f) return false;
    if (e0 == 0.0f && !owns(t.r0)) return false;
    if (e1 == 0.0f && !owns(t.r1)) return false;
    if (e2 == 0.0f && !owns(t.r2)) return false;
    const float num = e0 * t.z0 + e1 * t.z1 + e2 * t.z2, den = e0 * t.w0 + e1 * t.w1 + e2 * t.w2;
    if (!(den > 0.0f)) return false;   // the pixel sees the triangle's plane behind the eye (or all E = 0)
    z = num / den;
    if (z < 0.0f || z > 1.0f) return false;   // depth clipping (NaN passes here and never wins below)
    z = z + 0.0f;                              // -0 -> +0: the key's bit order needs z >= +0
    return true;
}

// ------------------------------------------------------------------------------------------------
// Alpha-masked materials (soc_rt.h "Alpha-masked materials"): the MASK forms of raster_small / raster_big
// ------------------------------------------------------------------------------------------------
// What a masked call adds to the two triangle kernels' arguments (the MASK = false forms take none of it).
struct MaskTable {
    const float* uvs;                // per vertex; a draw scene: per transformed-vertex slot
    const uint32_t* tri_materials;   // per triangle, or null (all 0)
    const soc_material* mats;
    int material_count;
};
// A triangle's share of the test: whether its material is flagged and, then, the fields the test reads and the uvs.
struct MaskTri {
    bool on;
    const char* data;   // level 0 of the albedo (null: alpha 1)
    int w, h, pitch;
    float cutoff, factor;
    float ua, va, ub, vb, uc, vc;
};
__device__ __forceinline__ MaskTable mask_of() { return MaskTable{nullptr, nullptr, nullptr, 0}; }
__device__ __forceinline__ MaskTable mask_of(const MaskTable& k) { return k; }

// UNIFORM (raster_big: the wave works on one triangle): `id` is wave-uniform, the material index goes through
// readfirstlane, so the index, material and uv fetches are scalar loads and the fields sit in SGPRs. Only the fields the
// test needs are read, and of an unflagged material only `flags`.
template <bool UNIFORM>
__device__ __forceinline__ MaskTri load_mask(const MaskTable& k, const uint32_t* __restrict__ idx, int id) {
    MaskTri m{};
    uint32_t mi = k.tri_materials ? min(k.tri_materials[id], (uint32_t)(k.material_count - 1)) : 0u;
    if (UNIFORM) mi = __builtin_amdgcn_readfirstlane(mi);
    const soc_material& mat = k.mats[mi];
    if (!(mat.flags & SOC_MATERIAL_ALPHA_MASK)) return m;
    m.on = true;
    m.data = static_cast<const char*>(mat.albedo.data);
    m.w = mat.albedo.width;
    m.h = mat.albedo.height;
    m.pitch = mat.albedo.pitch_bytes;
    m.cutoff = mat.alpha_cutoff;
    m.factor = mat.albedo_factor[3];
    const uint32_t a = idx[3 * id], b = idx[3 * id + 1], c = idx[3 * id + 2];
    m.ua = k.uvs[2 * a]; m.va = k.uvs[2 * a + 1];
    m.ub = k.uvs[2 * b]; m.vb = k.uvs[2 * b + 1];
    m.uc = k.uvs[2 * c]; m.vc = k.uvs[2 * c + 1];
    return m;
}

// Steps 1-5 of the contract for a covered fragment with edge values e0..e2: gbuffer_resolve's barycentrics and uv
// (same operands, same order, so the same bits), the level-0 REPEAT axes, two row loads, the exact integer bilinear of
// the four alpha bytes (<= 255 * 65536 < 2^24: the conversion is exact), one scale, one multiply, one compare.
__device__ __forceinline__ bool alpha_keeps(const MaskTri& m, float e0, float e1, float e2) {
#pragma clang fp contract(off)
    float alpha = 1.0f;
    if (m.data) {
        const float es = e0 + e1 + e2;
        const float b1 = e1 / es, b2 = e2 / es, b0 = 1.0f - b1 - b2;
        const float u = b0 * m.ua + b1 * m.ub + b2 * m.uc;
        const float v = b0 * m.va + b1 * m.vb + b2 * m.vc;
        const DImg im{const_cast<char*>(m.data), m.w, m.h, m.pitch};
        const Axis ax = axis_repeat_level(u, m.w), ay = axis_repeat_level(v, m.h);
        uint32_t t00, t10, t01, t11;
        texel_row_pair(im, ax.i0, ax.i1, ay.i0, t00, t10);
        texel_row_pair(im, ax.i0, ax.i1, ay.i1, t01, t11);
        const uint32_t kx = (uint32_t)(ax.w * 256.0f), ky = (uint32_t)(ay.w * 256.0f);
        const uint32_t A = ((t00 >> 24) * (256u - kx) + (t10 >> 24) * kx) * (256u - ky) +
                           ((t01 >> 24) * (256u - kx) + (t11 >> 24) * kx) * ky;
        alpha = (float)A * (1.0f / (255.0f * 65536.0f));
    }
    return alpha * m.factor >= m.cutoff;   // a NaN on either side: false, the fragment is discarded
}

// MASK: a fragment of a flagged triangle first reads the pixel's current value with a plain load. Stored values only
// decrease, so a stale (larger) value never skips a needed atomic; a value already below this fragment's key (depth-only:
// not above its biased depth bits) means the fragment has lost whatever its alpha, and it leaves before the taps. Then
// the test; a discarded fragment issues no atomic.
template <bool MASK>
__device__ __forceinline__ void shade(const TriSetup& t, int id, int x, int y, const RasterParams& p, void* target,
                                      size_t pitch, const MaskTri& mk) {
    float e0, e1, e2, z;
    if (!cover(t, x, y, e0, e1, e2, z)) return;
    // a plain load first: values only decrease, so a stale (larger) value never skips a needed atomic
    if (p.depth_only) {
#pragma clang fp contract(off)
        const float zb = fminf(fmaxf(z + t.bias, 0.0f), 1.0f);
        uint32_t* d = reinterpret_cast<uint32_t*>(static_cast<char*>(target) + (size_t)y * pitch) + x;
        const uint32_t key = __float_as_uint(zb);
        if (MASK && mk.on && (*d <= key || !alpha_keeps(mk, e0, e1, e2))) return;
        atomicMin(d, key);
    } else {
        const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)(0xFFFFFFFEu - (uint32_t)id);
        unsigned long long* d = reinterpret_cast<unsigned long long*>(static_cast<char*>(target) + (size_t)y * pitch) + x;
        if (MASK && mk.on && (*d < key || !alpha_keeps(mk, e0, e1, e2))) return;
        atomicMin(d, key);
    }
}

__device__ __forceinline__ TriSetup load_tri(const Workspace& ws, const uint32_t* __restrict__ idx, int id,
                                             const RasterParams& p) {
    const uint32_t a = idx[3 * id], b = idx[3 * id + 1], c = idx[3 * id + 2];
    return tri_setup(ws.screen[a], ws.screen[b], ws.screen[c], p);
}

__global__ __launch_bounds__(kWorkgroup) void raster_setup(const float* __restrict__ pos, Workspace ws, RasterParams p) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v == 0) *ws.counter = 0ull;
    if (v >= p.vertex_count) return;
    ws.screen[v] = clip_vertex(pos, v, p.model, p.vp, p.width, p.height);
}

__global__ __launch_bounds__(kWorkgroup) void raster_clear_vis(unsigned long long* vis, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) vis[i] = ((unsigned long long)__float_as_uint(1.0f) << 32) | KEY_EMPTY;
}

// One block row per image row: texels [0, width) of the row, never the bytes between the rows of a padded view.
__global__ __launch_bounds__(kWorkgroup) void raster_clear_depth(char* depth, size_t pitch, int width, int height) {
    const int x = (int)(blockIdx.x * 256 + threadIdx.x);
    if (x >= width) return;
    for (int y = (int)blockIdx.y; y < height; y += (int)gridDim.y)
        reinterpret_cast<float*>(depth + (size_t)y * pitch)[x] = 1.0f;
}

// The large triangles' entries are reserved once per workgroup: an LDS atomic gives each its offset in the workgroup's
// share and one global atomic on the packed counter reserves the share (one returning atomic on the one counter per
// wave cost ~40 us at 4K: the counter serialises them). The packed adds keep the entry slots and their tile ranges
// increasing together, as raster_big's search needs (SOC_RASTER_WG_ENTRIES=0: one atomic per wave, as before).
#ifndef SOC_RASTER_WG_ENTRIES
#define SOC_RASTER_WG_ENTRIES 1
#endif
// MASK = true takes one more argument, the MaskTable (M is empty otherwise: the MASK = false kernels keep their
// parameter lists and, as instantiations of these templates, their gfx950 instructions: profiles/alpha_mask_isa_identity.txt).
// Here the material is per lane: a flagged triangle's fields and uvs are fetched once, before its pixel loop.
template <bool MASK, typename... M>
__global__ __launch_bounds__(kWorkgroup) void raster_small(const uint32_t* __restrict__ idx, Workspace ws, RasterParams p,
                                                    void* target, size_t pitch, M... mask) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    TriSetup t{};
    t.live = false;
    if (id < p.triangle_count) t = load_tri(ws, idx, id, p);
    const int bw = t.px1 - t.px0 + 1, bh = t.py1 - t.py0 + 1;
    const bool big = t.live && (long long)bw * bh > p.small_pixels;
    if (SOC_RASTER_WG_ENTRIES) {
        __shared__ unsigned long long wg_acc, wg_base;
        if (threadIdx.x == 0) wg_acc = 0ull;
        __syncthreads();
        unsigned long long local = 0ull;
        if (big) {
            const uint32_t chunks = (uint32_t)(((bw + TILE - 1) / TILE) * ((bh + TILE - 1) / TILE));
            local = atomicAdd(&wg_acc, (1ull << ENTRY_SHIFT) + chunks);
        }
        __syncthreads();
        if (threadIdx.x == 0 && wg_acc) wg_base = atomicAdd(ws.counter, wg_acc);
        __syncthreads();
        if (big) {
            const unsigned long long old = wg_base + local;
            ws.entries[old >> ENTRY_SHIFT] = uint2{(uint32_t)id, (uint32_t)old};
            return;
        }
    } else if (big) {
        const uint32_t chunks = (uint32_t)(((bw + TILE - 1) / TILE) * ((bh + TILE - 1) / TILE));
        const unsigned long long old = atomicAdd(ws.counter, (1ull << ENTRY_SHIFT) + chunks);
        ws.entries[old >> ENTRY_SHIFT] = uint2{(uint32_t)id, (uint32_t)old};
        return;
    }
    if (!t.live) return;
    MaskTri mk{};
    if (MASK) mk = load_mask<false>(mask_of(mask...), idx, id);
    for (int y = t.py0; y <= t.py1; ++y)
        for (int x = t.px0; x <= t.px1; ++x) shade<MASK>(t, id, x, y, p, target, pitch, mk);
}

// Upper bound of the edge function over the pixel centres of [x0, x1] x [y0, y1] (a corner), minus a
// rounding margin: < 0 means no centre of the tile can pass this edge.
__device__ __forceinline__ float edge_max(f3 r, float x0, float x1, float y0, float y1) {
    const float m = fmaxf(fmaxf(edge(r, x0, y0), edge(r, x1, y0)), fmaxf(edge(r, x0, y1), edge(r, x1, y1)));
    const float slack = 1e-4f * (fabsf(r.x) * fmaxf(fabsf(x0), fabsf(x1)) + fabsf(r.y) * fmaxf(fabsf(y0), fabsf(y1)) + fabsf(r.z));
    return m + slack;
}

// One wave per work item (triangle, 32x32 tile of its box): 64 lanes, 2 rows per step.
// MASK: the wave's triangle, and so its material, is wave-uniform; its id goes through readfirstlane and load_mask<true>
// keeps the record on the scalar path. An unflagged triangle pays that one uniform branch, nothing per pixel.
template <bool MASK, typename... M>
__global__ __launch_bounds__(kWorkgroup) void raster_big(const uint32_t* __restrict__ idx, Workspace ws, RasterParams p,
                                                  void* target, size_t pitch, M... mask) {
    const unsigned long long c = *ws.counter;
    const uint32_t n_entries = (uint32_t)(c >> ENTRY_SHIFT), count = (uint32_t)(c & ((1ull << ENTRY_SHIFT) - 1));
    const int lane = threadIdx.x & 63;
    // each wave walks a contiguous slice of the work indices: one binary search for its first entry,
    // then the entry advances as the slice crosses tile ranges
    const uint32_t nwaves = gridDim.x * 4, wv = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t per = (count + nwaves - 1) / nwaves;
    const uint32_t begin = min(count, wv * per), end = min(count, begin + per);
    if (begin >= end) return;
    uint32_t lo = 0, hi = n_entries - 1;   // the last entry with first <= begin
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (ws.entries[mid].y <= begin) lo = mid;
        else hi = mid - 1;
    }
    uint32_t e_idx = lo;
    uint2 e = ws.entries[e_idx];
    uint32_t next_first = e_idx + 1 < n_entries ? ws.entries[e_idx + 1].y : 0xFFFFFFFFu;
    TriSetup t = load_tri(ws, idx, (int)e.x, p);
    MaskTri mk{};
    if (MASK) mk = load_mask<true>(mask_of(mask...), idx, (int)__builtin_amdgcn_readfirstlane(e.x));
    for (uint32_t it = begin; it < end; ++it) {
        if (it >= next_first) {
            do {
                ++e_idx;
                e = ws.entries[e_idx];
                next_first = e_idx + 1 < n_entries ? ws.entries[e_idx + 1].y : 0xFFFFFFFFu;
            } while (it >= next_first);
            t = load_tri(ws, idx, (int)e.x, p);
            if (MASK) mk = load_mask<true>(mask_of(mask...), idx, (int)__builtin_amdgcn_readfirstlane(e.x));
        }
        const uint2 item = uint2{e.x, it - e.y};
        const int tiles_x = (t.px1 - t.px0 + TILE) / TILE;
        const int ty = (int)item.y / tiles_x, tx = (int)item.y - ty * tiles_x;
        const int x0 = t.px0 + tx * TILE, y0 = t.py0 + ty * TILE;
        const int x1 = min(x0 + TILE - 1, t.px1), y1 = min(y0 + TILE - 1, t.py1);
        const float fx0 = (float)x0 + 0.5f, fx1 = (float)x1 + 0.5f, fy0 = (float)y0 + 0.5f, fy1 = (float)y1 + 0.5f;
        if (edge_max(t.r0, fx0, fx1, fy0, fy1) < 0.0f || edge_max(t.r1, fx0, fx1, fy0, fy1) < 0.0f ||
            edge_max(t.r2, fx0, fx1, fy0, fy1) < 0.0f)
            continue;
#if SOC_RASTER_FIXED_COLS
        const int x = x0 + (lane % TILE);
        if (x > x1) continue;
        for (int y = y0 + lane / TILE; y <= y1; y += 64 / TILE) shade<MASK>(t, (int)item.x, x, y, p, target, pitch, mk);
#else
        // the wave's lanes as cols x (64 / cols) pixels, cols the smallest power of two >= the item's width (4..TILE):
        // a narrow box (the median large triangle's is 14 x 15 pixels at 4K) keeps most lanes on its pixels
        const int cw = x1 - x0 + 1;
        const int lc = cw <= 4 ? 2 : cw <= 8 ? 3 : cw <= 16 ? 4 : 5;   // log2 cols (TILE = 32)
        const int x = x0 + (lane & ((1 << lc) - 1));
        if (x > x1) continue;
        for (int y = y0 + (lane >> lc); y <= y1; y += 64 >> lc) shade<MASK>(t, (int)item.x, x, y, p, target, pitch, mk);
#endif
    }
}

// ------------------------------------------------------------------------------------------------
// G-buffer resolve (g_buffer_generation.inl:161-225)
// ------------------------------------------------------------------------------------------------
struct ResolveParams {
    Mat4 model, vp, prev_vp;
    Mat3 normal3;
    int width, height, triangle_count, material_count;
    int tex_pairs;   // share the footprint of same-extent normal image + albedo (tuning knob SOC_GB_TEX_PAIRS, default on)
    int paired;      // read a material's paired_texels when it has them (tuning knob SOC_GB_PAIRED, default on)
    int wave_shape;  // pixels of a wave / workgroup: 0 = 64 x 1 / 64 x 4, 1 = 16 x 4 / 64 x 4, 2 = 8 x 8 / 32 x 8 (default),
                     // 3 = 8 x 8 / 16 x 16, 4 = 8 x 8 / 8 x 32 (tuning knob SOC_GB_WAVE)
};

__device__ __forceinline__ f3 mat3_vec_exact(const Mat3& M, f3 v) {
#pragma clang fp contract(off)
    const float* m = M.m;
    return f3{m[0] * v.x + m[3] * v.y + m[6] * v.z, m[1] * v.x + m[4] * v.y + m[7] * v.z, m[2] * v.x + m[5] * v.y + m[8] * v.z};
}

// Per-pixel normalize of the resolve (the interpolated normal and the TBN): v_rsq_f32 and three multiplies instead of the
// correctly rounded sqrt and three IEEE divisions (~40 VALU each, five per normal-mapped pixel). A few fp32 ulps against
// the oracle's normalize, stored as RGBA16F (the G-buffer tolerance); a zero vector still gives NaN. The per-vertex
// normal (gbuffer_vertex_setup) stays exact. SOC_GB_FAST_NORMALIZE=0 builds the exact form (A/B).
#ifndef SOC_GB_FAST_NORMALIZE
#define SOC_GB_FAST_NORMALIZE 1
#endif
__device__ __forceinline__ f3 normalize_exact(f3 a);
__device__ __forceinline__ f3 normalize_px(f3 a) {
#if SOC_GB_FAST_NORMALIZE
    const float k = __builtin_amdgcn_rsqf(__builtin_fmaf(a.z, a.z, __builtin_fmaf(a.y, a.y, a.x * a.x)));
    return f3{a.x * k, a.y * k, a.z * k};
#else
    return normalize_exact(a);
#endif
}
__device__ __forceinline__ f3 normalize_exact(f3 a) {
#pragma clang fp contract(off)
    const float l = sqrtf(a.x * a.x + a.y * a.y + a.z * a.z);
    return f3{a.x / l, a.y / l, a.z / l};
}

// The vertex stage of GBufferGeneration (g_buffer_generation.inl:169-178) for vertex v: the raster's
// homogeneous screen vertex, normalize(normal_matrix * normal), and the current / previous clip x, y, w.
// 4 float4 per vertex; computed once per vertex into the workspace (gbuffer_vertex_setup) or inline by
// the resolve; the same function either way, so both give the same bits.
struct VtxData { float4 s, n, cc, pc; };
// d by value: by reference, the two draws kernels (which call this from a lambda) came out with another schedule
__device__ __forceinline__ void store_vertex(float4* vd, int i, VtxData d) {
    vd[4 * i] = d.s;
    vd[4 * i + 1] = d.n;
    vd[4 * i + 2] = d.cc;
    vd[4 * i + 3] = d.pc;
}
// f32mat3x3(normal_matrix): the upper 3x3 of a column-major 4x4
__host__ __device__ __forceinline__ Mat3 normal3_of(const float m[16]) {
    return Mat3{{m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]}};
}

__device__ __forceinline__ VtxData vertex_data(const soc_mesh& mesh, uint32_t v, const ResolveParams& p) {
#pragma clang fp contract(off)
    VtxData d;
    d.s = clip_vertex(mesh.positions, v, p.model, p.vp, p.width, p.height);
    const float* nr = mesh.normals;
    const f3 n = normalize_exact(mat3_vec_exact(p.normal3, f3{nr[3 * v], nr[3 * v + 1], nr[3 * v + 2]}));
    d.n = float4{n.x, n.y, n.z, 0.0f};   // .w of n, cc, pc: the world position (the TBN's out_position)
    const float* ps = mesh.positions;
    const f4 wp = mat_vec_exact(p.model, ps[3 * v], ps[3 * v + 1], ps[3 * v + 2], 1.0f);
    const f4 c = mat_vec_exact(p.vp, wp.x, wp.y, wp.z, wp.w);
    const f4 q = mat_vec_exact(p.prev_vp, wp.x, wp.y, wp.z, wp.w);
    d.n.w = wp.x;
    d.cc = float4{c.x, c.y, c.w, wp.y};
    d.pc = float4{q.x, q.y, q.w, wp.z};
    return d;
}

// vertex_data with per-object motion (draw scenes): the previous clip position from the draw's model
// matrix of the PREVIOUS frame, prev_vp . (prev_model . p), the current chain's operations in its order; everything else
// is vertex_data's (pc.w stays the current world z). A prev_model equal to p.model bit for bit gives vertex_data's bits:
// the same operations on the same operands.
__device__ __forceinline__ VtxData vertex_data_motion(const soc_mesh& mesh, uint32_t v, const ResolveParams& p,
                                                      const Mat4& prev_model) {
#pragma clang fp contract(off)
    VtxData d = vertex_data(mesh, v, p);
    const float* ps = mesh.positions;
    const f4 wq = mat_vec_exact(prev_model, ps[3 * v], ps[3 * v + 1], ps[3 * v + 2], 1.0f);
    const f4 q = mat_vec_exact(p.prev_vp, wq.x, wq.y, wq.z, wq.w);
    d.pc = float4{q.x, q.y, q.w, d.pc.w};
    return d;
}

__global__ __launch_bounds__(kWorkgroup) void gbuffer_vertex_setup(soc_mesh mesh, float4* __restrict__ vd, ResolveParams p) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= mesh.vertex_count) return;
    store_vertex(vd, v, vertex_data(mesh, (uint32_t)v, p));
}

template <bool PRE>
__device__ __forceinline__ VtxData fetch_vertex(const soc_mesh& mesh, const float4* __restrict__ vd, uint32_t v,
                                                const ResolveParams& p) {
    if (!PRE) return vertex_data(mesh, v, p);
    return VtxData{vd[4 * v], vd[4 * v + 1], vd[4 * v + 2], vd[4 * v + 3]};
}

#ifndef SOC_GB_WAVES
#define SOC_GB_WAVES 5   // waves per SIMD the resolve's registers allow: 96 VGPRs, no spill (A/B builds: 1 = unconstrained)
#endif
// LAYER = false: the resolve (GBufferGeneration). LAYER = true: the same pixel code for a layer drawn over a G-buffer that
// is already there (soc_draw_terrain: DrawTerrain after GBufferGeneration, draw_terrain.inl: depth LOAD, LESS_OR_EQUAL,
// three colour attachments): a pixel with an empty key, or whose fragment lies behind the depth image's value, leaves
// before any index, vertex or texel fetch and writes nothing; a winning one writes depth, velocity, albedo and normal as
// the resolve computes them and never the emissive image (`emissive` is not touched; the launcher passes the albedo). One
// kernel template, not a shared __device__ function: inlined from a function, the two LAYER = false instantiations came out
// with other registers and three more instructions; as instantiations of this template their gfx950 instructions are
// those of the kernel before the parameter existed.
template <bool PRE, bool LAYER>
__global__ __launch_bounds__(kWorkgroup) __attribute__((amdgpu_waves_per_eu(SOC_GB_WAVES))) void gbuffer_resolve(soc_mesh mesh, const soc_material* __restrict__ mats,
                                                       const unsigned long long* __restrict__ vis, DImg depth,
                                                       DImg albedo, DImg emissive, DImg normal, DImg velocity,
                                                       const float4* __restrict__ vd, ResolveParams p) {
#pragma clang fp contract(off)
    __shared__ float lut[256];
    lut[threadIdx.y * 64 + threadIdx.x] = srgb_to_linear(unorm8(threadIdx.y * 64 + threadIdx.x));
    __syncthreads();
    // row-major tiles: the XCD-aware orders measured 13-40 % slower here (profiles/r04_probe_gbuffer_order.txt).
    // A wave covers 64 x 1 pixels (shape 0), 16 x 4 (1, the workgroup a 64 x 4 tile) or 8 x 8 (2: a 32 x 8 tile, the
    // default; 3: 16 x 16; 4: 8 x 32): a compact wave footprint shares the texture lines of the anisotropic taps in L1.
    const int lane = threadIdx.x, wave = threadIdx.y;
    int x, y;
    if (p.wave_shape == 1) {
        x = blockIdx.x * 64 + wave * 16 + (lane & 15);
        y = blockIdx.y * 4 + (lane >> 4);
    } else if (p.wave_shape == 2) {
        x = blockIdx.x * 32 + wave * 8 + (lane & 7);
        y = blockIdx.y * 8 + (lane >> 3);
    } else if (p.wave_shape == 3) {
        x = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
        y = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    } else if (p.wave_shape == 4) {
        x = blockIdx.x * 8 + (lane & 7);
        y = blockIdx.y * 32 + wave * 8 + (lane >> 3);
    } else {
        x = blockIdx.x * 64 + lane;
        y = blockIdx.y * 4 + wave;
    }
    if (x >= p.width || y >= p.height) return;
    const unsigned long long key = vis[(size_t)y * p.width + x];
    const uint32_t low = (uint32_t)key;
    if (LAYER) {
        if (low == KEY_EMPTY) return;
        // z_t <= z_e on the float bits (both >= +0, so the bits order like the values): ties go to the layer, the later draw
        if ((uint32_t)(key >> 32) > row_ptr<uint32_t>(depth, y)[x]) return;
    } else if (low == KEY_EMPTY) {   // clear values (g_buffer_generation.inl:78-100, depth cleared to 1.0)
        row_ptr_w<float>(depth, y)[x] = 1.0f;
        row_ptr_w<uint2>(albedo, y)[x] = pack_h4(f4{0.2f, 0.4f, 1.0f, 1.0f});
        row_ptr_w<uint2>(emissive, y)[x] = pack_h4(f4{0.0f, 0.0f, 0.0f, 1.0f});
        row_ptr_w<uint2>(normal, y)[x] = pack_h4(f4{0.0f, 0.0f, 0.0f, 1.0f});
        row_ptr_w<uint2>(velocity, y)[x] = pack_h4(f4{0.0f, 0.0f, 0.0f, 1.0f});
        return;
    }
    const int id = (int)(0xFFFFFFFEu - low);
    const uint32_t ia = mesh.indices[3 * id], ib = mesh.indices[3 * id + 1], ic = mesh.indices[3 * id + 2];
    const VtxData VA = fetch_vertex<PRE>(mesh, vd, ia, p), VB = fetch_vertex<PRE>(mesh, vd, ib, p),
                  VC = fetch_vertex<PRE>(mesh, vd, ic, p);
    const float4 A = VA.s, B = VB.s, C = VC.s;
    // perspective-correct barycentrics b_i = E_i / sum E from the raster's edge functions
    const f3 v0{A.x, A.y, A.w}, v1{B.x, B.y, B.w}, v2{C.x, C.y, C.w};
    f3 r0 = cross_exact(v1, v2), r1 = cross_exact(v2, v0), r2 = cross_exact(v0, v1);
    const float det = v0.x * r0.x + v0.y * r0.y + v0.z * r0.z;
    if (det < 0.0f) { r0 = -r0; r1 = -r1; r2 = -r2; }
    const float fx = (float)x + 0.5f, fy = (float)y + 0.5f;
    const float e0 = edge(r0, fx, fy), e1 = edge(r1, fx, fy), e2 = edge(r2, fx, fy);
    const float es = e0 + e1 + e2;
    const float b1 = e1 / es, b2 = e2 / es, b0 = 1.0f - b1 - b2;

    // interpolated vertex outputs (g_buffer_generation.inl:169-178)
    const float* uv = mesh.uvs;
    const float u = b0 * uv[2 * ia] + b1 * uv[2 * ib] + b2 * uv[2 * ic];
    const float v = b0 * uv[2 * ia + 1] + b1 * uv[2 * ib + 1] + b2 * uv[2 * ic + 1];
    const uint32_t mi = mesh.materials ? min(mesh.materials[id], (uint32_t)(p.material_count - 1)) : 0u;
    const soc_material& m = mats[mi];
    // velocity and depth first: the clip positions are dead before the texture taps (123 -> fewer live VGPRs there)
    {
        f4 vel = f4{0.0f, 0.0f, 0.0f, 0.0f};
        if (!(m.flags & SOC_MATERIAL_ZERO_VELOCITY)) {
            const float4 ca = VA.cc, cb = VB.cc, cd = VC.cc, pa = VA.pc, pb = VB.pc, pd = VC.pc;
            const float cx = b0 * ca.x + b1 * cb.x + b2 * cd.x, cy = b0 * ca.y + b1 * cb.y + b2 * cd.y;
            const float cw = b0 * ca.z + b1 * cb.z + b2 * cd.z;
            const float px = b0 * pa.x + b1 * pb.x + b2 * pd.x, py = b0 * pa.y + b1 * pb.y + b2 * pd.y;
            const float pw = b0 * pa.z + b1 * pb.z + b2 * pd.z;
            vel = f4{((cx / cw) * 0.5f + 0.5f) - ((px / pw) * 0.5f + 0.5f), ((cy / cw) * 0.5f + 0.5f) - ((py / pw) * 0.5f + 0.5f),
                     0.0f, 1.0f};
        }
        row_ptr_w<float>(depth, y)[x] = __uint_as_float((uint32_t)(key >> 32));
        row_ptr_w<uint2>(velocity, y)[x] = pack_h4(vel);
    }
    f3 n;
    if ((m.flags & SOC_MATERIAL_NORMAL_MAP) && m.normal_map.data) {   // draw_terrain.inl:206-219
        const DImg nm{static_cast<char*>(m.normal_map.data), m.normal_map.width, m.normal_map.height, m.normal_map.pitch_bytes};
        const f4 t = sample_h4(nm, u, v);
        n = normalize_px(f3{t.x, t.y, t.z});
    } else {
        const float4 na = VA.n, nb = VB.n, nc = VC.n;
        n = normalize_px(f3{b0 * na.x + b1 * nb.x + b2 * nc.x, b0 * na.y + b1 * nb.y + b2 * nc.y,
                               b0 * na.z + b1 * nb.z + b2 * nc.z});
    }
    const bool tbn = (m.flags & SOC_MATERIAL_NORMAL_TEXTURE) && m.normal_image.data;
    const bool mipped = m.flags & SOC_MATERIAL_MIPMAPPED;
    // fine dFdx / dFdy: this triangle's attributes at the two centres of the pixel's 2x2 quad per direction
    // (what helper invocations evaluate); world positions only for the TBN
    f3 Q1{0.0f, 0.0f, 0.0f}, Q2{0.0f, 0.0f, 0.0f};
    UVGrad gr{0.0f, 0.0f, 0.0f, 0.0f};
    if (tbn || mipped) {
        f4 wa{0.0f, 0.0f, 0.0f, 0.0f}, wb = wa, wc = wa;
        if (tbn) {   // vertex stage out_position (:171-172), kept by the vertex stage in the .w components
            wa = f4{VA.n.w, VA.cc.w, VA.pc.w, 1.0f};
            wb = f4{VB.n.w, VB.cc.w, VB.pc.w, 1.0f};
            wc = f4{VC.n.w, VC.cc.w, VC.pc.w, 1.0f};
        }
        auto attr = [&](float sx, float sy, f3& P, float& su, float& sv) {
            const float a0 = edge(r0, sx, sy), a1 = edge(r1, sx, sy), a2 = edge(r2, sx, sy);
            const float as = a0 + a1 + a2;
            const float c1 = a1 / as, c2 = a2 / as, c0 = 1.0f - c1 - c2;
            P = f3{c0 * wa.x + c1 * wb.x + c2 * wc.x, c0 * wa.y + c1 * wb.y + c2 * wc.y, c0 * wa.z + c1 * wb.z + c2 * wc.z};
            su = c0 * uv[2 * ia] + c1 * uv[2 * ib] + c2 * uv[2 * ic];
            sv = c0 * uv[2 * ia + 1] + c1 * uv[2 * ib + 1] + c2 * uv[2 * ic + 1];
        };
        const float qx = (float)(x & ~1) + 0.5f, qy = (float)(y & ~1) + 0.5f;
        f3 px0, px1, py0, py1;
        float ux0, vx0, ux1, vx1, uy0, vy0, uy1, vy1;
        attr(qx, fy, px0, ux0, vx0);
        attr(qx + 1.0f, fy, px1, ux1, vx1);
        attr(fx, qy, py0, uy0, vy0);
        attr(fx, qy + 1.0f, py1, uy1, vy1);
        Q1 = f3{px1.x - px0.x, px1.y - px0.y, px1.z - px0.z};
        Q2 = f3{py1.x - py0.x, py1.y - py0.y, py1.z - py0.z};
        gr = UVGrad{ux1 - ux0, vx1 - vx0, uy1 - uy0, vy1 - vy0};
    }
    auto tex = [&](const soc_img& t) {
        return mipped ? sample_texture_mip(t, u, v, gr, m.max_anisotropy, lut) : sample_texture(t, u, v, lut);
    };
    // normal image and albedo of one extent on the reference sampler: one footprint for both (same bits)
    const bool pair = tbn && mipped && p.tex_pairs && m.albedo.data && m.albedo.width == m.normal_image.width &&
                      m.albedo.height == m.normal_image.height;
    f4 t_pair{0.0f, 0.0f, 0.0f, 0.0f}, al_pair = t_pair;
    if (pair && (m.flags & SOC_MATERIAL_PAIRED_TEXELS) && m.paired_texels && p.paired)
        sample_texture_mip2p(m.normal_image, m.albedo, m.paired_texels, u, v, gr, m.max_anisotropy, lut, t_pair, al_pair);
    else if (pair)
        sample_texture_mip2(m.normal_image, m.albedo, u, v, gr, m.max_anisotropy, lut, t_pair, al_pair);
    if (tbn) {   // g_buffer_generation.inl:197-211
        const f4 t = pair ? t_pair : tex(m.normal_image);
        const f3 tn{t.x * 2.0f - 1.0f, t.y * 2.0f - 1.0f, t.z * 2.0f - 1.0f};
        const float st1t = gr.dvdx, st2t = gr.dvdy;
        const f3 N = normalize_px(n);
        const f3 T = normalize_px(f3{Q1.x * st2t - Q2.x * st1t, Q1.y * st2t - Q2.y * st1t, Q1.z * st2t - Q2.z * st1t});
        const f3 B = normalize_px(cross_exact(N, T));
        n = normalize_px(f3{T.x * tn.x + B.x * tn.y + N.x * tn.z, T.y * tn.x + B.y * tn.y + N.y * tn.z,
                               T.z * tn.x + B.z * tn.y + N.z * tn.z});
    }
    f3 em = f3{0.0f, 0.0f, 0.0f};
    if (m.has_emissive) {
        const f4 e = tex(m.emissive);
        em = f3{e.x * m.emissive_factor[0], e.y * m.emissive_factor[1], e.z * m.emissive_factor[2]};
    }
    const f4 al = pair ? al_pair : tex(m.albedo);
    row_ptr_w<uint2>(albedo, y)[x] = pack_h4(f4{al.x * m.albedo_factor[0] + em.x, al.y * m.albedo_factor[1] + em.y,
                                                al.z * m.albedo_factor[2] + em.z, 1.0f});
    if (!LAYER) row_ptr_w<uint2>(emissive, y)[x] = pack_h4(f4{em.x, em.y, em.z, 1.0f});
    row_ptr_w<uint2>(normal, y)[x] = pack_h4(f4{n.x, n.y, n.z, 1.0f});
}

// ------------------------------------------------------------------------------------------------
// Draw scenes (soc_rt.h "Draw scenes"): per-entity draws with their own transforms
// ------------------------------------------------------------------------------------------------
// The reference's draw loop (g_buffer_generation.inl:111-144, depth_prepass.inl, sun_shadow_draw.inl) as tables. The
// topology is static until the draws change, the transforms and so every transformed vertex change per frame:
//   load time  draws_build_slots  one lane per transformed-vertex slot (one per (draw, vertex of its range)):
//                                 {source vertex, transform} and the source vertex's uv
//              draws_build_tris   one lane per global triangle (draw order): validates its three fetched indices +
//                                 vertex_offset against the draw's vertex range, rebases them to the draw's slots and
//                                 writes the triangle's material
//   per frame  raster_setup_draws / gbuffer_vertex_setup_draws: raster_setup / gbuffer_vertex_setup per slot, with the
//                                 slot's source vertex and its draw's matrices (clip_vertex / vertex_data as they are);
//                                 gbuffer_vertex_setup_draws_motion: the same with the previous clip position from the
//                                 draw's model matrix of the previous frame (opt-in per-object motion vectors)
// raster_small, raster_big and gbuffer_resolve<true> then run UNCHANGED on a single-mesh view of the tables (slot count
// as the vertex count, the rebased indices, the slot uvs, the per-triangle materials): a triangle's global id is its
// position in the rebased index buffer, so the keys and the tie rule are the serial draw loop's.

struct DrawWorkspace {    // the draw-scene workspace (draw_layout, raster_host.hpp) as pointers
    uint32_t* flag;       // first failing draw (DRAWS_OK: none)
    uint2* slots;         // {source vertex, transform}
    float2* slot_uvs;
    uint32_t *indices, *materials;
    DrawRec* draws;
    void* view[2];        // 0: the camera (visibility, G-buffer vertex data), 1: the sun (depth)
};

DrawWorkspace draw_carve(void* ws, long long S, long long T, int32_t D) {
    char* p = static_cast<char*>(ws);
    const DrawLayout l = draw_layout(S, T, D);
    return DrawWorkspace{reinterpret_cast<uint32_t*>(p), reinterpret_cast<uint2*>(p + l.slots),
                         reinterpret_cast<float2*>(p + l.slot_uvs), reinterpret_cast<uint32_t*>(p + l.indices),
                         reinterpret_cast<uint32_t*>(p + l.materials), reinterpret_cast<DrawRec*>(p + l.draws),
                         {p + l.view[0], p + l.view[1]}};
}

// The last draw whose base (slot_base or triangle_base) is <= i. Empty draws share their base with the next draw, so
// the last one at a base is the draw that owns item i. n >= 1.
template <int32_t DrawRec::*BASE>
__device__ __forceinline__ int find_draw(const DrawRec* __restrict__ draws, int n, int i) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (draws[mid].*BASE <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kWorkgroup) void draws_build_slots(const float* __restrict__ uvs, DrawWorkspace ws, int draw_count,
                                                         int slot_count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= slot_count) return;
    const DrawRec d = ws.draws[find_draw<&DrawRec::slot_base>(ws.draws, draw_count, i)];
    // the host checked first_vertex + vertex_count <= the scene's vertex_count: src addresses the vertex arrays
    const uint32_t src = (uint32_t)(d.first_vertex + (i - d.slot_base));
    ws.slots[i] = uint2{src, (uint32_t)d.transform};
    if (uvs) ws.slot_uvs[i] = float2{uvs[2 * src], uvs[2 * src + 1]};
}

// Every read is bounded by what the host checked (first_index + 3 triangle_count <= index_count); the fetched index
// itself addresses nothing here: it is only compared and rebased. A triangle with an index outside its draw's vertex
// range records its draw (the smallest wins) and is written as a degenerate triangle of slot 0.
__global__ __launch_bounds__(kWorkgroup) void draws_build_tris(const uint32_t* __restrict__ indices, DrawWorkspace ws,
                                                        int draw_count, int triangle_count) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= triangle_count) return;
    const int di = find_draw<&DrawRec::triangle_base>(ws.draws, draw_count, id);
    const DrawRec d = ws.draws[di];
    const size_t at = (size_t)d.first_index + 3 * (size_t)(id - d.triangle_base);
    uint32_t out[3];
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        const long long v = (long long)indices[at + k] + d.vertex_offset - d.first_vertex;
        ok = ok && v >= 0 && v < d.vertex_count;
        out[k] = (uint32_t)(d.slot_base + (int)v);
    }
    if (!ok) {
        atomicMin(ws.flag, (uint32_t)di);
        out[0] = out[1] = out[2] = 0u;
    }
    ws.indices[3 * (size_t)id] = out[0];
    ws.indices[3 * (size_t)id + 1] = out[1];
    ws.indices[3 * (size_t)id + 2] = out[2];
    ws.materials[id] = (uint32_t)d.material;
}

// Calls f with the transform of this lane's slot. Consecutive slots of one draw share a transform: when every lane of
// the wave names the same one (a wave inside one draw), 32 lanes fetch its 32 floats once (one coalesced 128-byte load)
// into the wave's LDS record and every lane reads the matrices from there (broadcast reads); a wave that straddles draws
// loads per lane from global memory. The same values reach the same arithmetic either way. Every lane of the
// workgroup must call this, once per kernel (lanes past the last slot pass the last slot's transform). The explicit
// forms without LDS (a branch on a readfirstlane index, a waterfall loop over the wave's distinct transforms) do not
// survive the compiler: it folds both back into the per-lane load (SOC_DRAWS_LDS_TRANSFORM=0 builds that form: A/B).
#ifndef SOC_DRAWS_LDS_TRANSFORM
#define SOC_DRAWS_LDS_TRANSFORM 1
#endif
template <typename F>
__device__ __forceinline__ void with_slot_transform(const soc_transform* __restrict__ xf, uint32_t t, F&& f) {
#if !SOC_DRAWS_LDS_TRANSFORM
    f(xf[t]);
#else
    static_assert(sizeof(soc_transform) == 32 * sizeof(float), "one float per lane of half a wave");
    __shared__ soc_transform wave_xf[kWorkgroup / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t first = __builtin_amdgcn_readfirstlane(t);
    const bool uniform = __all(t == first);
    if (uniform && lane < 32)
        reinterpret_cast<float*>(&wave_xf[wave])[lane] = reinterpret_cast<const float*>(&xf[first])[lane];
    __syncthreads();
    if (uniform) f(wave_xf[wave]);
    else f(xf[t]);
#endif
}

__device__ __forceinline__ Mat4 mat4_of(const float* __restrict__ m) {
    Mat4 r;
    for (int i = 0; i < 16; ++i) r.m[i] = m[i];
    return r;
}

// raster_setup per transformed-vertex slot (p.vertex_count slots).
__global__ __launch_bounds__(kWorkgroup) void raster_setup_draws(const float* __restrict__ pos, const uint2* __restrict__ slots,
                                                          const soc_transform* __restrict__ xf, Workspace ws, RasterParams p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *ws.counter = 0ull;
    if (p.vertex_count == 0) return;
    const bool live = i < p.vertex_count;
    const uint2 sl = slots[live ? i : p.vertex_count - 1];
    with_slot_transform(xf, sl.y, [&](const soc_transform& t) {
        const float4 v = clip_vertex(pos, (int)sl.x, mat4_of(t.model_matrix), p.vp, p.width, p.height);
        if (live) ws.screen[i] = v;
    });
}

// gbuffer_vertex_setup per transformed-vertex slot: vertex_data of the slot's source vertex with its draw's model and
// normal matrix (mesh: the scene's vertex arrays).
__global__ __launch_bounds__(kWorkgroup) void gbuffer_vertex_setup_draws(soc_mesh mesh, const uint2* __restrict__ slots,
                                                                  const soc_transform* __restrict__ xf, int slot_count,
                                                                  float4* __restrict__ vd, ResolveParams p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (slot_count == 0) return;
    const bool live = i < slot_count;
    const uint2 sl = slots[live ? i : slot_count - 1];
    with_slot_transform(xf, sl.y, [&](const soc_transform& t) {
        ResolveParams q = p;
        q.model = mat4_of(t.model_matrix);
        q.normal3 = normal3_of(t.normal_matrix);
        const VtxData d = vertex_data(mesh, sl.x, q);
        if (live) store_vertex(vd, i, d);
    });
}

// The motion form of with_slot_transform (soc_gbuffer_resolve_draws_motion): f gets the slot's current transform and its
// draw's PREVIOUS model matrix (prev[t].model_matrix; the previous normal matrix is never read). A wave inside one draw
// fetches both in one load instruction, lanes 0-31 the current record's 32 floats and lanes 32-47 the previous model
// matrix's 16, into its LDS record (192 bytes per wave); a wave that straddles draws loads per lane. xf and prev may
// be the same array. The same rule: every lane of the workgroup calls this, once per kernel.
struct MotionXf {
    soc_transform cur;
    float prev_model[16];
};
template <typename F>
__device__ __forceinline__ void with_slot_transform_motion(const soc_transform* xf, const soc_transform* prev, uint32_t t,
                                                           F&& f) {
#if !SOC_DRAWS_LDS_TRANSFORM
    f(xf[t], prev[t].model_matrix);
#else
    static_assert(sizeof(MotionXf) == 48 * sizeof(float), "one float per lane of three quarters of a wave");
    __shared__ MotionXf wave_xf[kWorkgroup / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t first = __builtin_amdgcn_readfirstlane(t);
    const bool uniform = __all(t == first);
    if (uniform && lane < 48) {
        const float* src = lane < 32 ? reinterpret_cast<const float*>(&xf[first]) + lane : prev[first].model_matrix + (lane - 32);
        reinterpret_cast<float*>(&wave_xf[wave])[lane] = *src;
    }
    __syncthreads();
    if (uniform) f(wave_xf[wave].cur, wave_xf[wave].prev_model);
    else f(xf[t], prev[t].model_matrix);
#endif
}

// gbuffer_vertex_setup_draws with per-object motion: everything but pc as there (the same vertex_data, the same current
// matrices); pc from the draw's previous model matrix, its .w payload still the current world z.
__global__ __launch_bounds__(kWorkgroup) void gbuffer_vertex_setup_draws_motion(soc_mesh mesh, const uint2* __restrict__ slots,
                                                                         const soc_transform* xf, const soc_transform* prev,
                                                                         int slot_count, float4* __restrict__ vd,
                                                                         ResolveParams p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (slot_count == 0) return;
    const bool live = i < slot_count;
    const uint2 sl = slots[live ? i : slot_count - 1];
    with_slot_transform_motion(xf, prev, sl.y, [&](const soc_transform& t, const float* prev_model) {
        ResolveParams q = p;
        q.model = mat4_of(t.model_matrix);
        q.normal3 = normal3_of(t.normal_matrix);
        const VtxData d = vertex_data_motion(mesh, sl.x, q, mat4_of(prev_model));
        if (live) store_vertex(vd, i, d);
    });
}

// ------------------------------------------------------------------------------------------------
// Issuing: the clears, one raster ladder, one resolve
// ------------------------------------------------------------------------------------------------
void clear_visibility(uint64_t* visibility, int W, int H, hipStream_t s) {
    const size_t n = (size_t)W * H;
    launch("raster_clear_vis", kWorkgroup, raster_clear_vis, (unsigned)((n + 255) / 256), kWorkgroup, 0, s,
           reinterpret_cast<unsigned long long*>(visibility), n);
}
// depth clear 1.0 (sun_shadow_draw.inl:71-74): the width texels of each row only, a padded view's bytes between the rows
// belong to the caller
void clear_depth(const soc_img& depth, hipStream_t s) {
    launch("raster_clear_depth", kWorkgroup, raster_clear_depth, dim3(ceil_div(depth.width, 256), min(depth.height, 65535)),
           kWorkgroup, 0, s, static_cast<char*>(depth.data), (size_t)depth.pitch_bytes, depth.width, depth.height);
}

// Where a raster call's triangles come from, with the raster workspace of (V, T) to use: a mesh (raster_setup with its
// model matrix) or a built draw scene's tables (slots: raster_setup_draws per slot, each with its transform's model matrix;
// p.model stays zero).
struct RasterSource {
    const float *positions, *model;
    const uint32_t* indices;
    int V, T;
    void* workspace;
    const uint2* slots;
    const soc_transform* transforms;
};
RasterSource mesh_source(const soc_mesh* m, void* workspace) {
    return RasterSource{m->positions, m->model_matrix, m->indices, m->vertex_count, m->triangle_count, workspace, nullptr, nullptr};
}
RasterSource draws_source(const soc_draw_scene* sc, const DrawTotals& tot, int view) {
    const DrawWorkspace dw = draw_carve(sc->workspace, tot.slots, tot.triangles, sc->draw_count);
    return RasterSource{sc->positions, nullptr, dw.indices, (int)tot.slots, (int)tot.triangles, dw.view[view], dw.slots, sc->transforms};
}

// The alpha test's table for each source: the mesh's own uvs and per-triangle materials, or the built scene's slot uvs and
// its per-triangle material table.
MaskTable mesh_mask(const soc_mesh* m, const soc_material* d_materials, int32_t material_count) {
    return MaskTable{m->uvs, m->materials, d_materials, material_count};
}
MaskTable draws_mask(const soc_draw_scene* sc, const DrawTotals& tot, const soc_material* d_materials, int32_t material_count) {
    const DrawWorkspace dw = draw_carve(sc->workspace, tot.slots, tot.triangles, sc->draw_count);
    return MaskTable{reinterpret_cast<const float*>(dw.slot_uvs), dw.materials, d_materials, material_count};
}

// The vertex kernel, raster_small and raster_big into a W x H target: the visibility buffer (bias null) or, depth-only, a
// D32 image with the Vulkan depth bias {constant, slope}.
// mask: the MASK forms of the two triangle kernels with this table (null: the forms every unmasked call launches).
int issue_raster(const RasterSource& src, const float* vp, int cull, void* target, size_t pitch, int W, int H, const float* bias,
                 hipStream_t s, const char* pass, const MaskTable* mask = nullptr) {
    // model, vp, width, height, vertex_count, triangle_count, cull, depth_only, bias_constant, bias_slope, small_pixels
    const RasterParams p{src.model ? mat4(src.model) : Mat4{}, mat4(vp), W, H, src.V, src.T, cull, bias ? 1 : 0,
                         bias ? bias[0] : 0.0f, bias ? bias[1] : 0.0f, SMALL_PIXELS};
    Workspace ws = carve(src.workspace, src.V, src.T);
    const unsigned blocks = ceil_div(max(src.V, 1), 256);
    if (!src.slots) launch("raster_setup", kWorkgroup, raster_setup, blocks, kWorkgroup, 0, s, src.positions, ws, p);
    else launch("raster_setup_draws", kWorkgroup, raster_setup_draws, blocks, kWorkgroup, 0, s, src.positions, src.slots, src.transforms, ws, p);
    if (src.T > 0 && !mask) {
        launch("raster_small", kWorkgroup, raster_small<false>, ceil_div(src.T, 256), kWorkgroup, 0, s, src.indices, ws, p, target, pitch);
        launch("raster_big", kWorkgroup, raster_big<false>, 2048, kWorkgroup, 0, s, src.indices, ws, p, target, pitch);
    } else if (src.T > 0) {
        launch("raster_small_masked", kWorkgroup, raster_small<true, MaskTable>, ceil_div(src.T, 256), kWorkgroup, 0, s, src.indices,
               ws, p, target, pitch, *mask);
        launch("raster_big_masked", kWorkgroup, raster_big<true, MaskTable>, 2048, kWorkgroup, 0, s, src.indices, ws, p, target,
               pitch, *mask);
    }
    return check_launch(pass);
}

struct GBufferImages { soc_img depth, albedo, emissive, normal, velocity; };

// The checks, parameters and launch geometry every resolve shares: everything of ResolveParams but the matrices of the
// mesh (model, normal3) and its triangle count.
int resolve_prepare(const char* pass, const soc_globals* g, const soc_material* d_materials, int32_t material_count,
                    const uint64_t* visibility, const GBufferImages& im, ResolveParams& p, dim3& grd) {
    const soc_img* colour[4] = {&im.albedo, &im.emissive, &im.normal, &im.velocity};
    const char* what[4] = {"albedo", "emissive", "normal", "velocity"};
    int rc = check_img(im.depth, SOC_FMT_D32F, pass, "depth");
    for (int i = 0; i < 4 && !rc; ++i) rc = check_img(*colour[i], SOC_FMT_RGBA16F, pass, what[i]);
    if (rc) return rc;
    if (!g || !d_materials || material_count <= 0 || !visibility)
        return set_error(SOC_E_INVALID_ARG, "%s: null globals / materials / visibility", pass);
    const int W = im.depth.width, H = im.depth.height;
    for (const soc_img* i : colour)
        if (i->width != W || i->height != H)
            return set_error(SOC_E_SHAPE, "%s: G-buffer images must share the depth extent", pass);
    p.vp = mat4(g->camera_projection_view_matrix);
    p.prev_vp = mat4(g->camera_previous_projection_view_matrix);
    p.width = W;
    p.height = H;
    p.material_count = material_count;
    p.tex_pairs = tuning_knob("SOC_GB_TEX_PAIRS", 1);
    p.paired = tuning_knob("SOC_GB_PAIRED", 1);
    p.wave_shape = tuning_knob("SOC_GB_WAVE", 2);   // 8 x 8-pixel waves: 687 -> 626 us at 4K (profiles/r04_probe_gbuffer_wave.txt)
    grd = dim3(ceil_div(W, 64), ceil_div(H, 4));
    if (p.wave_shape == 2) grd = dim3(ceil_div(W, 32), ceil_div(H, 8));
    else if (p.wave_shape == 3) grd = dim3(ceil_div(W, 16), ceil_div(H, 16));
    else if (p.wave_shape == 4) grd = dim3(ceil_div(W, 8), ceil_div(H, 32));
    else if (p.wave_shape != 0 && p.wave_shape != 1) return set_error(SOC_E_INVALID_ARG, "%s: SOC_GB_WAVE %d", pass, p.wave_shape);
    return SOC_OK;
}
void set_mesh_matrices(ResolveParams& p, const soc_mesh* mesh) {
    p.model = mat4(mesh->model_matrix);
    p.normal3 = normal3_of(mesh->normal_matrix);
    p.triangle_count = mesh->triangle_count;
}

// Who computes the per-vertex data the resolve reads: gbuffer_vertex_setup over a mesh (slots null), its draws form per
// slot, or that one's motion form (previous: last frame's transforms). vdata null: nobody, the resolve computes
// vertex_data inline (PRE = false).
struct VertexStage {
    soc_mesh src;   // the vertex arrays
    int count;      // vertices or slots
    float4* vdata;
    const uint2* slots;
    const soc_transform *transforms, *previous;
};
VertexStage mesh_stage(const soc_mesh* mesh, void* workspace) {
    float4* vdata = workspace ? carve(workspace, mesh->vertex_count, mesh->triangle_count).vdata : nullptr;
    return VertexStage{*mesh, mesh->vertex_count, vdata, nullptr, nullptr, nullptr};
}

// The vertex stage, then gbuffer_resolve<PRE, LAYER> over `mesh` (what the pixels read: indices, uvs, materials).
int issue_resolve(const char* pass, const VertexStage& vs, const soc_mesh& mesh, bool layer, const soc_material* d_materials,
                  const uint64_t* visibility, const GBufferImages& im, const ResolveParams& p, dim3 grd, hipStream_t s) {
    const bool stage = vs.vdata && vs.count > 0;
    const unsigned blocks = ceil_div(max(vs.count, 1), 256);
    if (stage && !vs.slots)
        launch("gbuffer_vertex_setup", kWorkgroup, gbuffer_vertex_setup, blocks, kWorkgroup, 0, s, vs.src, vs.vdata, p);
    else if (stage && vs.previous)
        launch("gbuffer_vertex_setup_draws_motion", kWorkgroup, gbuffer_vertex_setup_draws_motion, blocks, kWorkgroup, 0, s, vs.src,
               vs.slots, vs.transforms, vs.previous, vs.count, vs.vdata, p);
    else if (stage)
        launch("gbuffer_vertex_setup_draws", kWorkgroup, gbuffer_vertex_setup_draws, blocks, kWorkgroup, 0, s, vs.src, vs.slots,
               vs.transforms, vs.count, vs.vdata, p);
    // named in the order the three kernels have always been emitted in (this compiler follows the first naming)
    auto* kernel = gbuffer_resolve<true, false>;
    if (!vs.vdata) kernel = gbuffer_resolve<false, false>;
    else if (layer) kernel = gbuffer_resolve<true, true>;
    launch(layer ? "gbuffer_resolve_layer" : "gbuffer_resolve", kWorkgroup, kernel, grd, dim3(64, 4), 0, s, mesh, d_materials,
           reinterpret_cast<const unsigned long long*>(visibility), dimg(im.depth), dimg(im.albedo), dimg(im.emissive),
           dimg(im.normal), dimg(im.velocity), vs.vdata, p);
    return check_launch(pass);
}

}  // namespace
}  // namespace soc

using namespace soc;

// soc_raster_visibility / _depth and their _masked twins (masked: with the table's checks, then the MASK kernels)
static int mesh_visibility(const char* name, const char* pass, const soc_mesh* mesh, const float* view_projection, int32_t cull,
                           uint64_t* visibility, int32_t width, int32_t height, int32_t clear, void* workspace, bool masked,
                           const soc_material* d_materials, int32_t material_count, soc_stream stream) {
    int rc = check_mesh(mesh, name, false);
    if (rc) return rc;
    if (!view_projection || !visibility || !workspace || width <= 0 || height <= 0 || cull < 0 || cull > 2)
        return set_error(SOC_E_INVALID_ARG, "%s: null argument, bad extent or cull mode", name);
    if (masked && (rc = check_mask_table(d_materials, material_count, mesh->uvs, 0, name))) return rc;
    const MaskTable mask = masked ? mesh_mask(mesh, d_materials, material_count) : MaskTable{};
    hipStream_t s = hs(stream);
    if (clear) clear_visibility(visibility, width, height, s);
    return issue_raster(mesh_source(mesh, workspace), view_projection, cull, visibility, (size_t)width * 8, width, height, nullptr,
                        s, pass, masked ? &mask : nullptr);
}
static int mesh_depth(const char* name, const char* pass, const soc_mesh* mesh, const float* view_projection, int32_t cull,
                      float bias_constant, float bias_slope, soc_img depth, void* workspace, bool masked,
                      const soc_material* d_materials, int32_t material_count, soc_stream stream) {
    int rc = check_mesh(mesh, name, false);
    if (!rc) rc = check_img(depth, SOC_FMT_D32F, name, "depth");
    if (rc) return rc;
    if (!view_projection || !workspace || cull < 0 || cull > 2)
        return set_error(SOC_E_INVALID_ARG, "%s: null argument or bad cull mode", name);
    if (masked && (rc = check_mask_table(d_materials, material_count, mesh->uvs, 0, name))) return rc;
    const MaskTable mask = masked ? mesh_mask(mesh, d_materials, material_count) : MaskTable{};
    hipStream_t s = hs(stream);
    clear_depth(depth, s);
    const float bias[2] = {bias_constant, bias_slope};
    return issue_raster(mesh_source(mesh, workspace), view_projection, cull, depth.data, (size_t)depth.pitch_bytes, depth.width,
                        depth.height, bias, s, pass, masked ? &mask : nullptr);
}

extern "C" int soc_raster_visibility(const soc_mesh* mesh, const float view_projection[16], int32_t cull,
                                     uint64_t* visibility, int32_t width, int32_t height, int32_t clear,
                                     void* workspace, soc_stream stream) {
    return mesh_visibility("soc_raster_visibility", "raster_visibility", mesh, view_projection, cull, visibility, width, height,
                           clear, workspace, false, nullptr, 0, stream);
}
extern "C" int soc_raster_visibility_masked(const soc_mesh* mesh, const float view_projection[16], int32_t cull,
                                            uint64_t* visibility, int32_t width, int32_t height, int32_t clear, void* workspace,
                                            const soc_material* d_materials, int32_t material_count, soc_stream stream) {
    return mesh_visibility("soc_raster_visibility_masked", "raster_visibility_masked", mesh, view_projection, cull, visibility,
                           width, height, clear, workspace, true, d_materials, material_count, stream);
}

extern "C" int soc_raster_depth(const soc_mesh* mesh, const float view_projection[16], int32_t cull, float bias_constant,
                                float bias_slope, soc_img depth, void* workspace, soc_stream stream) {
    return mesh_depth("soc_raster_depth", "raster_depth", mesh, view_projection, cull, bias_constant, bias_slope, depth, workspace,
                      false, nullptr, 0, stream);
}
extern "C" int soc_raster_depth_masked(const soc_mesh* mesh, const float view_projection[16], int32_t cull, float bias_constant,
                                       float bias_slope, soc_img depth, void* workspace, const soc_material* d_materials,
                                       int32_t material_count, soc_stream stream) {
    return mesh_depth("soc_raster_depth_masked", "raster_depth_masked", mesh, view_projection, cull, bias_constant, bias_slope,
                      depth, workspace, true, d_materials, material_count, stream);
}

extern "C" int soc_gbuffer_resolve(const soc_globals* g, const soc_mesh* mesh, const soc_material* d_materials,
                                   int32_t material_count, const uint64_t* visibility, soc_img depth, soc_img albedo,
                                   soc_img emissive, soc_img normal, soc_img velocity, void* workspace,
                                   soc_stream stream) {
    int rc = check_mesh(mesh, "soc_gbuffer_resolve", true);
    if (rc) return rc;
    const GBufferImages im{depth, albedo, emissive, normal, velocity};
    ResolveParams p{};
    dim3 grd;
    rc = resolve_prepare("soc_gbuffer_resolve", g, d_materials, material_count, visibility, im, p, grd);
    if (rc) return rc;
    set_mesh_matrices(p, mesh);
    // with a workspace: per-vertex outputs once, then the per-pixel resolve reads them
    return issue_resolve("gbuffer_resolve", mesh_stage(mesh, workspace), *mesh, false, d_materials, visibility, im, p, grd, hs(stream));
}

// ------------------------------------------------------------------------------------------------
// Terrain layer: DrawTerrain / SunShadowDrawTerrain over what the entity tasks left (soc_rt.h "Terrain layer")
// ------------------------------------------------------------------------------------------------
extern "C" int soc_draw_terrain(const soc_globals* g, const soc_mesh* mesh, const soc_material* d_materials,
                                int32_t material_count, uint64_t* visibility, soc_img depth, soc_img albedo, soc_img normal,
                                soc_img velocity, void* workspace, soc_stream stream) {
    const char* name = "soc_draw_terrain";
    int rc = check_mesh(mesh, name, true);
    if (rc) return rc;
    if (!workspace) return set_error(SOC_E_INVALID_ARG, "%s: null workspace (the layer always uses the per-vertex workspace)", name);
    // DrawTerrain has no emissive attachment (draw_terrain.inl:14-17): the albedo stands in, for the shared checks and in
    // the launch (the LAYER form never touches it)
    const GBufferImages im{depth, albedo, albedo, normal, velocity};
    ResolveParams p{};
    dim3 grd;
    rc = resolve_prepare(name, g, d_materials, material_count, visibility, im, p, grd);
    if (rc) return rc;
    // the layer always runs 8 x 8-pixel waves, whatever SOC_GB_WAVE asked for
    p.wave_shape = 2;
    grd = dim3(ceil_div(depth.width, 32), ceil_div(depth.height, 8));
    set_mesh_matrices(p, mesh);
    hipStream_t s = hs(stream);
    clear_visibility(visibility, depth.width, depth.height, s);
    rc = issue_raster(mesh_source(mesh, workspace), g->camera_projection_view_matrix, SOC_CULL_FRONT, visibility,
                      (size_t)depth.width * 8, depth.width, depth.height, nullptr, s, "draw_terrain");
    if (rc) return rc;
    return issue_resolve("draw_terrain", mesh_stage(mesh, workspace), *mesh, true, d_materials, visibility, im, p, grd, s);
}

extern "C" int soc_sun_shadow_draw_terrain(const soc_mesh* mesh, const float view_projection[16], int32_t clear, soc_img depth,
                                           void* workspace, soc_stream stream) {
    const char* name = "soc_sun_shadow_draw_terrain";
    int rc = check_mesh(mesh, name, false);
    if (!rc) rc = check_img(depth, SOC_FMT_D32F, name, "depth");
    if (rc) return rc;
    if (!view_projection || !workspace) return set_error(SOC_E_INVALID_ARG, "%s: null view_projection or workspace", name);
    hipStream_t s = hs(stream);
    if (clear) clear_depth(depth, s);   // a frame whose head draws no shadow: the clear SunShadowDraw would have made
    const float no_bias[2] = {0.0f, 0.0f};   // sun_shadow_draw_terrain.inl:47-58: cull BACK and no depth bias
    return issue_raster(mesh_source(mesh, workspace), view_projection, SOC_CULL_BACK, depth.data, (size_t)depth.pitch_bytes,
                        depth.width, depth.height, no_bias, s, "sun_shadow_draw_terrain");
}

// ------------------------------------------------------------------------------------------------
// Draw scenes: entry points
// ------------------------------------------------------------------------------------------------
extern "C" int soc_draw_scene_build(const soc_draw_scene* scene, soc_stream stream) {
    DrawTotals tot;
    int rc = check_draw_scene(scene, "soc_draw_scene_build", false, tot);
    if (rc) return rc;
    soc_draw_scene_release(scene);   // until this build has finished the workspace holds no built scene
    const int D = scene->draw_count, S = (int)tot.slots, T = (int)tot.triangles;
    const DrawWorkspace dw = draw_carve(scene->workspace, tot.slots, tot.triangles, D);
    std::vector<DrawRec> recs((size_t)D);
    int32_t slot_base = 0, triangle_base = 0;
    for (int i = 0; i < D; ++i) {
        const soc_draw& d = scene->draws[i];
        recs[i] = DrawRec{d.first_index, d.triangle_count, d.vertex_offset, d.first_vertex, d.vertex_count, d.transform,
                          d.material, slot_base, triangle_base};
        slot_base += d.vertex_count;
        triangle_base += d.triangle_count;
    }
    hipStream_t s = hs(stream);
    uint32_t failed = DRAWS_OK;
    // recs and failed live on this frame's stack: the stream is synchronised before it returns
    bool ok = hipMemsetAsync(dw.flag, 0xFF, 256, s) == hipSuccess;
    if (ok && D > 0) ok = hipMemcpyAsync(dw.draws, recs.data(), (size_t)D * sizeof(DrawRec), hipMemcpyHostToDevice, s) == hipSuccess;
    if (ok && S > 0)
        launch("draws_build_slots", kWorkgroup, draws_build_slots, ceil_div(S, 256), kWorkgroup, 0, s, scene->uvs, dw, D, S);
    if (ok && T > 0)
        launch("draws_build_tris", kWorkgroup, draws_build_tris, ceil_div(T, 256), kWorkgroup, 0, s, scene->indices, dw, D, T);
    if (ok) rc = check_launch("soc_draw_scene_build");
    if (ok && !rc) ok = hipMemcpyAsync(&failed, dw.flag, sizeof failed, hipMemcpyDeviceToHost, s) == hipSuccess;
    const bool synced = hipStreamSynchronize(s) == hipSuccess;
    if (rc) return rc;
    if (!ok || !synced) {
        (void)hipGetLastError();
        return set_error(SOC_E_HIP, "soc_draw_scene_build: copying the draw tables or reading the validation flag failed");
    }
    record_built_scene(scene, failed);
    if (failed != DRAWS_OK) {
        const soc_draw& d = scene->draws[failed];
        return set_error(SOC_E_SHAPE, "soc_draw_scene_build: draw %u fetches an index that, with vertex_offset %d, lies outside "
                         "its vertex range [%d, %d)", failed, d.vertex_offset, d.first_vertex, d.first_vertex + d.vertex_count);
    }
    return SOC_OK;
}

static int draws_visibility(const char* name, const char* pass, const soc_draw_scene* scene, const float* view_projection,
                            int32_t cull, uint64_t* visibility, int32_t width, int32_t height, int32_t clear, bool masked,
                            const soc_material* d_materials, int32_t material_count, soc_stream stream) {
    DrawTotals tot;
    // a masked call: the scene's description and the table first, so that every refusal that needs no build record comes
    // before the one that does
    int rc = masked ? check_draw_scene(scene, name, false, tot) : (int)SOC_OK;
    if (!rc && masked) rc = check_mask_table(d_materials, material_count, scene->uvs, scene->material_count, name);
    if (!rc) rc = check_built_scene(scene, name, false, tot);
    if (rc) return rc;
    if (!view_projection || !visibility || width <= 0 || height <= 0 || cull < 0 || cull > 2)
        return set_error(SOC_E_INVALID_ARG, "%s: null argument, bad extent or cull mode", name);
    const MaskTable mask = masked ? draws_mask(scene, tot, d_materials, material_count) : MaskTable{};
    hipStream_t s = hs(stream);
    if (clear) clear_visibility(visibility, width, height, s);
    return issue_raster(draws_source(scene, tot, 0), view_projection, cull, visibility, (size_t)width * 8, width, height, nullptr, s,
                        pass, masked ? &mask : nullptr);
}
static int draws_depth(const char* name, const char* pass, const soc_draw_scene* scene, const float* view_projection, int32_t cull,
                       float bias_constant, float bias_slope, soc_img depth, bool masked, const soc_material* d_materials,
                       int32_t material_count, soc_stream stream) {
    DrawTotals tot;
    int rc = masked ? check_draw_scene(scene, name, false, tot) : (int)SOC_OK;   // the order: see draws_visibility
    if (!rc && masked) rc = check_mask_table(d_materials, material_count, scene->uvs, scene->material_count, name);
    if (!rc) rc = check_built_scene(scene, name, false, tot);
    if (!rc) rc = check_img(depth, SOC_FMT_D32F, name, "depth");
    if (rc) return rc;
    if (!view_projection || cull < 0 || cull > 2)
        return set_error(SOC_E_INVALID_ARG, "%s: null argument or bad cull mode", name);
    const MaskTable mask = masked ? draws_mask(scene, tot, d_materials, material_count) : MaskTable{};
    hipStream_t s = hs(stream);
    clear_depth(depth, s);
    const float bias[2] = {bias_constant, bias_slope};
    return issue_raster(draws_source(scene, tot, 1), view_projection, cull, depth.data, (size_t)depth.pitch_bytes, depth.width,
                        depth.height, bias, s, pass, masked ? &mask : nullptr);
}

extern "C" int soc_raster_visibility_draws(const soc_draw_scene* scene, const float view_projection[16], int32_t cull,
                                           uint64_t* visibility, int32_t width, int32_t height, int32_t clear,
                                           soc_stream stream) {
    return draws_visibility("soc_raster_visibility_draws", "raster_visibility_draws", scene, view_projection, cull, visibility,
                            width, height, clear, false, nullptr, 0, stream);
}
extern "C" int soc_raster_visibility_draws_masked(const soc_draw_scene* scene, const float view_projection[16], int32_t cull,
                                                  uint64_t* visibility, int32_t width, int32_t height, int32_t clear,
                                                  const soc_material* d_materials, int32_t material_count, soc_stream stream) {
    return draws_visibility("soc_raster_visibility_draws_masked", "raster_visibility_draws_masked", scene, view_projection, cull,
                            visibility, width, height, clear, true, d_materials, material_count, stream);
}

extern "C" int soc_raster_depth_draws(const soc_draw_scene* scene, const float view_projection[16], int32_t cull,
                                      float bias_constant, float bias_slope, soc_img depth, soc_stream stream) {
    return draws_depth("soc_raster_depth_draws", "raster_depth_draws", scene, view_projection, cull, bias_constant, bias_slope,
                       depth, false, nullptr, 0, stream);
}
extern "C" int soc_raster_depth_draws_masked(const soc_draw_scene* scene, const float view_projection[16], int32_t cull,
                                             float bias_constant, float bias_slope, soc_img depth,
                                             const soc_material* d_materials, int32_t material_count, soc_stream stream) {
    return draws_depth("soc_raster_depth_draws_masked", "raster_depth_draws_masked", scene, view_projection, cull, bias_constant,
                       bias_slope, depth, true, d_materials, material_count, stream);
}

// soc_gbuffer_resolve_draws (previous null) and soc_gbuffer_resolve_draws_motion: the same checks, tables and resolve; the
// vertex stage is gbuffer_vertex_setup_draws or its motion form.
static int resolve_draws(const char* name, const char* pass, const soc_globals* g, const soc_draw_scene* scene,
                         const soc_transform* previous, const soc_material* d_materials, int32_t material_count,
                         const uint64_t* visibility, const GBufferImages& im, soc_stream stream) {
    DrawTotals tot;
    int rc = check_built_scene(scene, name, true, tot);
    if (rc) return rc;
    ResolveParams p{};   // model and normal3 stay zero: the vertex stage takes each slot's from its transform
    dim3 grd;
    rc = resolve_prepare(name, g, d_materials, material_count, visibility, im, p, grd);
    if (rc) return rc;
    if (material_count < scene->material_count)
        return set_error(SOC_E_SHAPE, "%s: %d materials, the scene's draws name up to %d", name, material_count,
                         scene->material_count);
    const int S = (int)tot.slots, T = (int)tot.triangles;
    p.triangle_count = T;
    const DrawWorkspace dw = draw_carve(scene->workspace, tot.slots, tot.triangles, scene->draw_count);
    // the scene's vertex arrays for the vertex stage; the tables as one mesh for the resolve (it reads the indices, the
    // uvs by slot, the materials and the per-slot vertex data only)
    soc_mesh src{};
    src.positions = scene->positions;
    src.normals = scene->normals;
    src.vertex_count = scene->vertex_count;
    soc_mesh view{};
    view.uvs = reinterpret_cast<const float*>(dw.slot_uvs);
    view.indices = dw.indices;
    view.materials = dw.materials;
    view.vertex_count = S;
    view.triangle_count = T;
    const VertexStage vs{src, S, carve(dw.view[0], S, T).vdata, dw.slots, scene->transforms, previous};
    return issue_resolve(pass, vs, view, false, d_materials, visibility, im, p, grd, hs(stream));
}

extern "C" int soc_gbuffer_resolve_draws(const soc_globals* g, const soc_draw_scene* scene, const soc_material* d_materials,
                                         int32_t material_count, const uint64_t* visibility, soc_img depth, soc_img albedo,
                                         soc_img emissive, soc_img normal, soc_img velocity, soc_stream stream) {
    return resolve_draws("soc_gbuffer_resolve_draws", "gbuffer_resolve_draws", g, scene, nullptr, d_materials, material_count,
                         visibility, GBufferImages{depth, albedo, emissive, normal, velocity}, stream);
}

extern "C" int soc_gbuffer_resolve_draws_motion(const soc_globals* g, const soc_draw_scene* scene,
                                                const soc_transform* previous_transforms, const soc_material* d_materials,
                                                int32_t material_count, const uint64_t* visibility, soc_img depth,
                                                soc_img albedo, soc_img emissive, soc_img normal, soc_img velocity,
                                                soc_stream stream) {
    if (!previous_transforms)
        return set_error(SOC_E_INVALID_ARG, "soc_gbuffer_resolve_draws_motion: null previous_transforms");
    return resolve_draws("soc_gbuffer_resolve_draws_motion", "gbuffer_resolve_draws_motion", g, scene, previous_transforms,
                         d_materials, material_count, visibility, GBufferImages{depth, albedo, emissive, normal, velocity}, stream);
}
