// A cloud's uniform grid as the kernels read it (include/roreg_hip.h "v6c"; built by csrc/icp.hip): the 64-byte descriptor, the records in
// cell order, the table of cell starts, the cell arithmetic and the walk over the cells a ball meets.  Shared by csrc/icp.hip and
// csrc/fpfh.hip; each definition fixes which records a kernel visits and in which order, so each is defined once.
#pragma once
#include "common.h"

namespace {

using GridDesc = roreg_icp_grid_desc;
static_assert(sizeof(GridDesc) == 64, "the grid buffer's records start 64 bytes in");

__device__ __forceinline__ const GridDesc *grid_desc(const void *g) { return reinterpret_cast<const GridDesc *>(g); }
__device__ __forceinline__ const float4 *grid_recs(const void *g) { return reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(g) + 64); }
__device__ __forceinline__ const int32_t *grid_starts(const void *g, int n) {
    return reinterpret_cast<const int32_t *>(reinterpret_cast<const char *>(g) + 64 + (size_t)n * 16);
}

// Cell coordinate along one axis, as a double: monotone in v (a rounded subtraction and a rounded multiplication by a positive constant are
// monotone), which is all the search's sufficiency argument needs.
__device__ __forceinline__ double cell_coord(double v, double o, double inv) { return floor((v - o) * inv); }
__device__ __forceinline__ int cell_clamp(double c, int dim) { return (int)fmin(fmax(c, 0.0), (double)(dim - 1)); }     // NaN -> 0
__device__ __forceinline__ int cell_of(const GridDesc &d, double inv, float x, float y, float z) {
    const int cx = cell_clamp(cell_coord((double)x, d.origin[0], inv), d.dims[0]);
    const int cy = cell_clamp(cell_coord((double)y, d.origin[1], inv), d.dims[1]);
    const int cz = cell_clamp(cell_coord((double)z, d.origin[2], inv), d.dims[2]);
    return (cz * d.dims[1] + cy) * d.dims[0] + cx;
}

// The records of every cell a ball of `reach` around (x, y, z) meets, ascending cell and ascending original row inside a cell (x-contiguous
// cells are one run of records, as in the search).  The coordinates are finite (a grid refuses a cloud that has others).
template <class F>
__device__ __forceinline__ void walk_ball(const GridDesc &g, const float4 *__restrict__ rec, const int32_t *__restrict__ st, double inv, double x, double y,
                                          double z, double reach, F f) {
    const int x0 = cell_clamp(cell_coord(x - reach, g.origin[0], inv), g.dims[0]), x1 = cell_clamp(cell_coord(x + reach, g.origin[0], inv), g.dims[0]);
    const int y0 = cell_clamp(cell_coord(y - reach, g.origin[1], inv), g.dims[1]), y1 = cell_clamp(cell_coord(y + reach, g.origin[1], inv), g.dims[1]);
    const int z0 = cell_clamp(cell_coord(z - reach, g.origin[2], inv), g.dims[2]), z1 = cell_clamp(cell_coord(z + reach, g.origin[2], inv), g.dims[2]);
    for (int cz = z0; cz <= z1; ++cz)
        for (int cy = y0; cy <= y1; ++cy) {
            const size_t c = ((size_t)cz * g.dims[1] + cy) * g.dims[0];
            const int b = max(st[c + x0], 0), e = min(st[c + x1 + 1], g.n);
            for (int k = b; k < e; ++k) f(rec[k]);
        }
}

}  // namespace
