// swt_rows.h -- the launch geometry of the row kernels (rows_kernel, pack_rows_kernel, mlm_kernel, decode_kernel): plain C++ with
// no HIP in it, so that the host compiler can sweep it (tests/rowshape_check.cpp).  A row gets a group of g lanes, a lane four
// columns a step; a wavefront holds 64 / g rows at a time and walks several such sets.
#pragma once

#include <cstdint>

namespace swt {

constexpr uint32_t kBtQuad = 4;             // columns of one lane per step
constexpr uint32_t kBtCols = 64 * kBtQuad;  // columns of one wavefront per step
constexpr uint64_t kBtMaxGrid = 1u << 20;   // workgroups of a launch at most

// The lanes of a row: the smallest power of two that covers the width at kBtQuad columns a lane, 64 where none does (such a row
// takes several steps).
inline uint32_t bt_group(uint32_t width) {
  uint32_t group = 1;
  while (group < 64 && (uint64_t)group * kBtQuad < width) group *= 2;
  return group;
}

// The sets of rows a wavefront walks and the workgroups of the launch, for `rows` rows under workgroups of `waves` wavefronts:
// one set where a row fills a quarter of a wavefront or more, four where rows are narrow, doubled while the grid would exceed
// kBtMaxGrid.  The last workgroup may run past the rows: the kernels mask.
struct RowShape {
  uint64_t sets;
  uint32_t grid;
};
inline RowShape bt_shape(uint64_t rows, uint32_t group, uint32_t waves) {
  const uint64_t per_set = (uint64_t)waves * (64 / group);  // rows of a workgroup in one set
  uint64_t sets = group >= 16 ? 1 : 4;
  while ((rows + per_set * sets - 1) / (per_set * sets) > kBtMaxGrid) sets *= 2;
  return RowShape{sets, (uint32_t)((rows + per_set * sets - 1) / (per_set * sets))};
}

}  // namespace swt
