// stream_host.h -- what the two streamline translation units share on the host
// (streamlines.cpp defines it, block_streamlines.cpp uses it): the checks of a
// tube, a colour table and a set's totals, the ring table, the lines of a host
// restatement and their expansion into tubes, the per-point scratch of the
// tube forms.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "job_arena.h"
#include "spray_rt.h"
#include "stream_kernels.h"

namespace spray_rt {
namespace strmhost {

constexpr uint64_t kMaxGridPoints = uint64_t(1) << 31;
constexpr uint64_t kMaxSeeds = uint64_t(1) << 31;

// What is wrong with a tube, a colour table or a set of totals (nullptr: nothing).
const char* tube_error(const spray_rt_tube& t);
const char* color_table_error(const uint32_t* table_rgb, int32_t ntable, float lo, float hi,
                              float* scale);
const char* totals_error(uint64_t npoints, uint64_t nverts, uint64_t nfaces);
// ... with the parameters of a trace (step, max_steps, direction, min_speed).
const char* trace_error(float step, int32_t max_steps, int32_t direction, float min_speed);

void ring_table(int nsides, float out[][2]);

// The lines of a host restatement: per point the position, frame normal,
// tangent and colour; per line the offsets and the info pair.
struct HostLines {
  std::vector<float> P, N, T;
  std::vector<uint32_t> col, off, info;
  uint64_t npoints = 0, tube_points = 0, tube_lines = 0;
};

// The tubes of emitted lines into the outputs that are not null.
void tubes_host(const HostLines& L, const spray_rt_tube& tube, float* verts_out,
                float* vnormals_out, uint32_t* colors_out, uint32_t* faces_out);

// The per-point and per-line scratch of the tube forms, laid out in M (of
// d_isomesh) for a counted field of nseeds seeds.
struct TubeScratch {
  detail::Take<float> points, pnormals, ptangents;
  detail::Take<uint32_t> pcolors, line_offsets, tube_points, tube_lines;
};
void take_tube_scratch(detail::Layout* M, size_t nseeds, const StreamRec& rec, TubeScratch* t);
void set_tube_scratch(StreamOut* O, const TubeScratch& t, void* base, const StreamRec& rec);

}  // namespace strmhost
}  // namespace spray_rt
