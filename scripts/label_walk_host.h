// Host replay of the run walk of biapy_amd/csrc/label_walk.h (lw_walk_runs), step for step, for the check programs (regionprops_cpu_check.cpp,
// shapeprops_cpu_check.cpp): one wave's span [begin, end) in trips of 256, the wave's shuffles and ballots as plain loops over its 64 lanes;
// everything that decides a run or its coordinates is the shared code of regionprops_core.h / overlap_core.h.  `g` has the volume's Y, X and
// n_max; `emit(label, z, y, x0, L)` receives every finished run of a label > 0 once.  A label is read only below `end` and through a checked
// access: an address outside the volume ends the run.
#pragma once
#include <algorithm>
#include <vector>

#include "regionprops_core.h"

template <class Geom, class Emit>
static void lw_walk_runs_host(const std::vector<int32_t>& labels, const Geom& g, int64_t begin, int64_t end, Emit&& emit) {
  const RpStride stride = rp_stride(g.Y, g.X);
  RpRun run{RP_NO_LABEL, 0, 0, 0, 0};
  RpPos at[OVL_LANES];
  for (int l = 0; l < OVL_LANES; ++l) at[l] = rp_pos_of((uint32_t)(begin + OVL_VPL * l), g.Y, g.X);
  for (int64_t t = begin; t < end; t += OVL_TRIP) {
    const uint32_t valid = (uint32_t)std::min<int64_t>(OVL_TRIP, end - t);
    int32_t lab[OVL_LANES][OVL_VPL];
    RpPos pos[OVL_LANES][OVL_VPL];
    for (int l = 0; l < OVL_LANES; ++l)
      for (int e = 0; e < OVL_VPL; ++e) {
        const int64_t i = t + OVL_VPL * l + e;
        lab[l][e] = rp_label(i < end ? labels.at((size_t)i) : 0, g.n_max);               // lw_load4: 0 past the end
        if (e) { pos[l][e] = pos[l][e - 1]; rp_step(pos[l][e], g.Y, g.X); } else pos[l][0] = at[l];
      }
    uint64_t H[OVL_VPL] = {0, 0, 0, 0};
    for (int l = 0; l < OVL_LANES; ++l)
      for (int e = 0; e < OVL_VPL; ++e) {
        const int32_t prev = e ? lab[l][e - 1] : l ? lab[l - 1][OVL_VPL - 1] : run.label;
        if ((uint32_t)(OVL_VPL * l + e) < valid && rp_is_head(lab[l][e], prev, pos[l][e].x)) H[e] |= (uint64_t)1 << l;
      }
    const bool any = (H[0] | H[1] | H[2] | H[3]) != 0;
    uint32_t first = 0, last = 0;
    int32_t last_label = 0;
    RpPos last_pos{0, 0, 0};
    if (any) {
      first = ovl_first_head(H);
      last = ovl_last_head(H);
      for (int l = 0; l < OVL_LANES; ++l)
        for (int e = 0; e < OVL_VPL; ++e) {
          const uint32_t p = (uint32_t)(OVL_VPL * l + e);
          if (((H[e] >> l) & 1) && p != last && lab[l][e] > 0)
            emit(lab[l][e], pos[l][e].z, pos[l][e].y, pos[l][e].x, ovl_next_head(H, l, e, valid) - p);
        }
      last_label = lab[last / OVL_VPL][last % OVL_VPL];
      last_pos = pos[last / OVL_VPL][last % OVL_VPL];
    }
    RpRun done{RP_NO_LABEL, 0, 0, 0, 0};
    if (rp_carry_step(run, done, any, first, last, last_label, last_pos, valid)) emit(done.label, done.z, done.y, done.x0, done.count);
    for (int l = 0; l < OVL_LANES; ++l) rp_advance(at[l], stride, g.Y, g.X);
  }
  if (run.count != 0 && run.label > 0) emit(run.label, run.z, run.y, run.x0, run.count);
}
