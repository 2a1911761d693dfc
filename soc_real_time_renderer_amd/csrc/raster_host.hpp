// raster_host.hpp — the host half of the raster entry points (raster_host.cpp, no HIP call): argument checks over the
// caller's arrays, the two workspace layouts, and the record of built draw scenes. raster.hip issues the launches.
#pragma once

#include "../../include/soc_rt.h"

namespace soc {

// Single-mesh raster workspace of V vertices and T triangles, as byte offsets (the base is 256-byte aligned):
//   [float4 screen vertices[V]] [u64 counter, pad to 256] [uint2 entries[T]] [float4 vertex data[4 V]]
struct RasterLayout { size_t counter, entries, vdata, bytes; };
RasterLayout raster_layout(int32_t V, int32_t T);

struct DrawRec {   // device copy of a draw with its prefix sums
    int32_t first_index, triangle_count, vertex_offset, first_vertex, vertex_count, transform, material;
    int32_t slot_base, triangle_base;
};
// Draw-scene workspace of S slots, T triangles and D draws, as byte offsets:
//   [u32 first failing draw (DRAWS_OK: none), pad to 256] [uint2 slots[S]] [float2 slot uvs[S]]
//   [u32 rebased indices[3 T]] [u32 triangle materials[T]] [DrawRec[D]] [raster workspace of (S, T)] x 2 views
struct DrawLayout { size_t slots, slot_uvs, indices, materials, draws, view[2], bytes; };
DrawLayout draw_layout(long long S, long long T, int32_t D);
constexpr uint32_t DRAWS_OK = 0xFFFFFFFFu;

int check_mesh(const soc_mesh* mesh, const char* pass, bool attributes);

// What a *_masked call adds to its twin's checks: the material table, the uvs the alpha test interpolates and, for a
// draw scene, a table that covers every draw's material (scene_materials; 0 for a mesh).
int check_mask_table(const soc_material* d_materials, int32_t material_count, const float* uvs, int32_t scene_materials,
                     const char* pass);

struct DrawTotals { long long slots = 0, triangles = 0; };
// Slot and triangle totals of a draw list; false on a null list, a negative count or field, or totals beyond int32.
bool draw_totals(const soc_draw* draws, int32_t draw_count, DrawTotals& t);
// Everything the host can check of a draw scene, before any HIP call.
int check_draw_scene(const soc_draw_scene* sc, const char* pass, bool attributes, DrawTotals& tot);
// check_draw_scene, then the build record of the workspace: only a scene whose build succeeded, unchanged since.
int check_built_scene(const soc_draw_scene* sc, const char* pass, bool attributes, DrawTotals& tot);
// soc_draw_scene_build finished: remembers what the workspace's tables were built from and the first draw the device
// validation rejected (DRAWS_OK: none), until soc_draw_scene_release or the next build.
void record_built_scene(const soc_draw_scene* sc, uint32_t failed_draw);

}  // namespace soc
