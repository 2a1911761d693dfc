// raster_host.cpp — what the raster entry points (raster.hip) decide before any HIP call: the checks of a mesh and of a
// draw scene (pointer and range arithmetic over the caller's arrays), the workspace layouts with their size functions, and
// the record of built draw scenes. No HIP call here: tools/sanitize builds this file under ASAN + UBSAN for san_host.
#include "raster_host.hpp"

#include <mutex>
#include <unordered_map>

#include "soc_internal.hpp"

namespace soc {
namespace {

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// What the library remembers of a built workspace: a fingerprint of everything the static tables were built from and
// the first draw the device validation rejected (DRAWS_OK: none).
struct DrawBuilt { uint64_t fingerprint; uint32_t failed_draw; };
std::mutex g_draws_mutex;
std::unordered_map<const void*, DrawBuilt> g_draws_built;

uint64_t fnv1a(uint64_t h, const void* data, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(data);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}
uint64_t draw_fingerprint(const soc_draw_scene* sc) {
    uint64_t h = 14695981039346656037ull;
    h = fnv1a(h, &sc->indices, sizeof sc->indices);
    h = fnv1a(h, &sc->uvs, sizeof sc->uvs);
    h = fnv1a(h, &sc->vertex_count, sizeof sc->vertex_count);
    h = fnv1a(h, &sc->index_count, sizeof sc->index_count);
    h = fnv1a(h, &sc->draw_count, sizeof sc->draw_count);
    if (sc->draw_count > 0) h = fnv1a(h, sc->draws, (size_t)sc->draw_count * sizeof(soc_draw));
    return h;
}

}  // namespace

RasterLayout raster_layout(int32_t V, int32_t T) {
    const size_t counter = align_up((size_t)V * 16, 256), entries = counter + 256, vdata = align_up(entries + (size_t)T * 8, 256);
    return RasterLayout{counter, entries, vdata, vdata + (size_t)V * 64};
}

DrawLayout draw_layout(long long S, long long T, int32_t D) {
    DrawLayout l;
    l.slots = 256;
    l.slot_uvs = align_up(l.slots + (size_t)S * 8, 256);
    l.indices = align_up(l.slot_uvs + (size_t)S * 8, 256);
    l.materials = align_up(l.indices + (size_t)T * 12, 256);
    l.draws = align_up(l.materials + (size_t)T * 4, 256);
    l.view[0] = align_up(l.draws + (size_t)D * sizeof(DrawRec), 256);
    const size_t view = align_up(raster_layout((int32_t)S, (int32_t)T).bytes, 256);
    l.view[1] = l.view[0] + view;
    l.bytes = l.view[1] + view;
    return l;
}

int check_mesh(const soc_mesh* mesh, const char* pass, bool attributes) {
    if (!mesh || !mesh->positions || !mesh->indices || mesh->vertex_count < 0 || mesh->triangle_count < 0)
        return set_error(SOC_E_INVALID_ARG, "%s: null mesh / positions / indices or negative counts", pass);
    if (attributes && (!mesh->normals || !mesh->uvs))
        return set_error(SOC_E_INVALID_ARG, "%s: the G-buffer resolve needs normals and uvs", pass);
    if ((uint32_t)mesh->triangle_count >= 0xFFFFFFFEu)
        return set_error(SOC_E_SHAPE, "%s: too many triangles for the visibility key", pass);
    return SOC_OK;
}

int check_mask_table(const soc_material* d_materials, int32_t material_count, const float* uvs, int32_t scene_materials,
                     const char* pass) {
    if (!d_materials || material_count <= 0)
        return set_error(SOC_E_INVALID_ARG, "%s: null materials or material_count %d <= 0", pass, material_count);
    if (!uvs) return set_error(SOC_E_INVALID_ARG, "%s: the alpha test needs uvs", pass);
    if (material_count < scene_materials)
        return set_error(SOC_E_INVALID_ARG, "%s: %d materials, the scene's draws name up to %d", pass, material_count,
                         scene_materials);
    return SOC_OK;
}

bool draw_totals(const soc_draw* draws, int32_t draw_count, DrawTotals& t) {
    if (draw_count < 0 || (draw_count > 0 && !draws)) return false;
    for (int32_t d = 0; d < draw_count; ++d) {
        if (draws[d].triangle_count < 0 || draws[d].vertex_count < 0 || draws[d].first_vertex < 0 || draws[d].first_index < 0)
            return false;
        t.slots += draws[d].vertex_count;
        t.triangles += draws[d].triangle_count;
    }
    return t.slots <= 0x7FFFFFFFll && t.triangles <= 0x7FFFFFFFll;
}

int check_draw_scene(const soc_draw_scene* sc, const char* pass, bool attributes, DrawTotals& tot) {
    if (!sc) return set_error(SOC_E_INVALID_ARG, "%s: null scene", pass);
    if (!sc->positions || !sc->indices || !sc->transforms || !sc->workspace || sc->vertex_count < 0 || sc->index_count < 0 ||
        sc->draw_count < 0 || (sc->draw_count > 0 && !sc->draws) || sc->transform_count <= 0 || sc->material_count <= 0)
        return set_error(SOC_E_INVALID_ARG, "%s: null positions / indices / draws / transforms / workspace or bad counts", pass);
    if (attributes && (!sc->normals || !sc->uvs))
        return set_error(SOC_E_INVALID_ARG, "%s: the G-buffer resolve needs normals and uvs", pass);
    if (reinterpret_cast<uintptr_t>(sc->workspace) % 256)
        return set_error(SOC_E_INVALID_ARG, "%s: the workspace must be 256-byte aligned", pass);
    long long triangles = 0;
    for (int32_t i = 0; i < sc->draw_count; ++i) {
        const soc_draw& d = sc->draws[i];
        if (d.triangle_count < 0 || d.vertex_count < 0 || d.first_vertex < 0 || d.first_index < 0)
            return set_error(SOC_E_INVALID_ARG, "%s: draw %d: negative first_index, triangle_count or vertex range", pass, i);
        if ((long long)d.first_index + 3ll * d.triangle_count > sc->index_count)
            return set_error(SOC_E_SHAPE, "%s: draw %d: first_index %d + 3 x %d triangles exceed index_count %d", pass, i,
                             d.first_index, d.triangle_count, sc->index_count);
        if ((long long)d.first_vertex + d.vertex_count > sc->vertex_count)
            return set_error(SOC_E_SHAPE, "%s: draw %d: vertex range [%d, %d + %d) exceeds vertex_count %d", pass, i,
                             d.first_vertex, d.first_vertex, d.vertex_count, sc->vertex_count);
        if (d.transform < 0 || d.transform >= sc->transform_count)
            return set_error(SOC_E_SHAPE, "%s: draw %d: transform %d outside the %d transforms", pass, i, d.transform,
                             sc->transform_count);
        if (d.material < 0 || d.material >= sc->material_count)
            return set_error(SOC_E_SHAPE, "%s: draw %d: material %d outside the %d materials", pass, i, d.material,
                             sc->material_count);
        triangles += d.triangle_count;
        if (triangles >= 0xFFFFFFFEll)
            return set_error(SOC_E_SHAPE, "%s: too many triangles for the visibility key", pass);
    }
    tot = DrawTotals();
    if (!draw_totals(sc->draws, sc->draw_count, tot))
        return set_error(SOC_E_SHAPE, "%s: more than 2^31 - 1 triangles or transformed vertices", pass);
    return SOC_OK;
}

int check_built_scene(const soc_draw_scene* sc, const char* pass, bool attributes, DrawTotals& tot) {
    int rc = check_draw_scene(sc, pass, attributes, tot);
    if (rc) return rc;
    DrawBuilt b{};
    {
        std::lock_guard<std::mutex> lock(g_draws_mutex);
        const auto it = g_draws_built.find(sc->workspace);
        if (it == g_draws_built.end())
            return set_error(SOC_E_INVALID_ARG, "%s: the scene's workspace was not built (soc_draw_scene_build)", pass);
        b = it->second;
    }
    if (b.fingerprint != draw_fingerprint(sc))
        return set_error(SOC_E_INVALID_ARG, "%s: the draws, indices or uvs changed since soc_draw_scene_build", pass);
    if (b.failed_draw != DRAWS_OK)
        return set_error(SOC_E_SHAPE, "%s: the scene failed its build: draw %u fetches an index outside its vertex range", pass,
                         b.failed_draw);
    return SOC_OK;
}

void record_built_scene(const soc_draw_scene* sc, uint32_t failed_draw) {
    std::lock_guard<std::mutex> lock(g_draws_mutex);
    g_draws_built[sc->workspace] = DrawBuilt{draw_fingerprint(sc), failed_draw};
}

}  // namespace soc

using namespace soc;

extern "C" size_t soc_raster_workspace_size(int32_t vertex_count, int32_t triangle_count) {
    if (vertex_count < 0 || triangle_count < 0) return 0;
    return raster_layout(vertex_count, triangle_count).bytes;
}

extern "C" size_t soc_draw_workspace_size(const soc_draw* draws, int32_t draw_count) {
    DrawTotals t;
    if (!draw_totals(draws, draw_count, t)) return 0;
    return draw_layout(t.slots, t.triangles, draw_count).bytes;
}

extern "C" void soc_draw_scene_release(const soc_draw_scene* scene) {
    if (!scene || !scene->workspace) return;
    std::lock_guard<std::mutex> lock(g_draws_mutex);
    g_draws_built.erase(scene->workspace);
}
