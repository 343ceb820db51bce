// tet_pipeline.h -- the device extraction of tet_isosurface.cpp below its C
// wrappers: count, weld, emit, then caller buffers or slots.  Entered here by
// the extractions that make their tets on the device (cell_isosurface.cpp), so
// that messages name the caller's mesh.
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <vector>

#include "rt_ctx.h"
#include "spray_rt.h"
#include "tet_kernels.h"

namespace spray_rt {
namespace detail {

struct TetCall {
  using Clock = std::chrono::steady_clock;
  const char* what = "tet isosurface";  // the call the messages name
  HeadTake<TetJob> jobs;  // in the context's tet arena
  HeadTake<uint32_t> status, offsets;
  HeadTake<TetRec> recs;
  HeadTake<TetInst> insts;
  HeadTake<TetOut> outs;
  size_t m_status = 0, m_rec = 0, m_insts = 0, m_outs = 0;  // the marks in front of them
  uint32_t max_blocks = 0, max_iblocks = 0;
  unsigned key_bits = 0;  // of the widest mesh's keys
  bool staged = false;    // some array came from host memory
  std::vector<TetRec> rec;
  Clock::time_point t0 = Clock::now();  // the phase times of spray_rt_tet_phase_times
};

// What is wrong with a mesh's colour map (nullptr: nothing; a mesh without a
// colour field has none); *scale = cmap::map_scale's.
const char* tet_color_error(const spray_rt_grid_color* gc, float* scale);

// Validates the meshes (and their colour maps, gcolors nullptr: none), runs the
// count pass and its scan and reads status and totals: host read 1.
// want_normals[i]: the call reads mesh i's point_normals.  Messages name the
// mesh, and its slot where slots is given.
int tet_count(spray_rt_ctx* c, int n, const spray_rt_tetmesh* meshes,
              const spray_rt_grid_color* gcolors, const int* slots,
              const std::vector<char>& want_normals, TetCall* call);
// Keys, the sort and the run count of a counted call, then the vertex counts:
// host read 2.
int tet_weld(spray_rt_ctx* c, int n, TetCall* call);
// The vertex and face passes of a welded call into outs[n].  The call's tables
// and instance scratch (TetInst: sorted keys, block bases, in-block ids) stay
// as they are until the next tet or cell extraction of the context.
int tet_emit(spray_rt_ctx* c, int n, const TetCall& call, const std::vector<TetOut>& outs);
// A welded call into the caller's buffers (spray_rt_tet_isosurface's arguments).
int tet_to_buffers(spray_rt_ctx* c, int n, const TetCall& call, float* const* verts,
                   float* const* vnormals, uint32_t* const* colors, uint32_t* const* faces,
                   const size_t* cap_verts, const size_t* cap_faces, size_t* nverts_out,
                   size_t* nfaces_out);
// A welded call into context scratch at the exact sizes, then the device build
// into slots; mesh i carries normals / colours where want_normals[i] /
// want_colors[i].
int tet_to_slots(spray_rt_ctx* c, int n, const int* slots, const TetCall& call,
                 const std::vector<char>& want_normals, const std::vector<char>& want_colors,
                 float* d_bounds, size_t* nfaces_out);
// What is wrong with the slot list of a call named what (0: nothing).
int tet_slots_error(spray_rt_ctx* c, const char* what, int n, const int* slots);
// cell_isosurface.cpp's extraction up to the tet pipeline's second host read,
// for a call named what: the cell pass (host read 1), the split of the crossing
// cells, tet_count and tet_weld on them.
int cell_weld(spray_rt_ctx* c, const char* what, int n, const spray_rt_cellmesh* meshes,
              const spray_rt_grid_color* gcolors, const int* slots,
              const std::vector<char>& want_normals, TetCall* call);

}  // namespace detail
}  // namespace spray_rt
