// 3D obstacles from geometry for gfx950: sphere, box and a triangle-mesh voxeliser.  Every kernel writes TypeObstacle
// into the cells it finds inside, whatever they held, and touches no other cell -- the rule of geometry_kernel (fnx_stencils.hip).
// Cell (i, j, k) sits at the point (x, y, z) = (i, j, k), as in createCylinder.
//
// The voxeliser marks the cells whose point lies inside a closed surface by the even-odd rule along x.  Its meaning is an exact rule
// (tests/voxel_reference.py states it in numpy and the GPU tests hold the kernels to it on every cell):
//   snap      q = rint(double(v) * 64); a face with an index outside [0, V), a non-finite coordinate or |q| > 2^20 is bad and skipped
//   cover     face (a, b, c) covers the row (j, k), p = (64 j, 64 k), iff an odd number of its edges, projected to (y, z), are crossed:
//             edge (a, b) is crossed iff (a.z > p.z) != (b.z > p.z) and, the ends ordered so that a.z < b.z,
//             (b.y - a.y) (p.z - a.z) - (p.y - a.y) (b.z - a.z) > 0.  Exact in int64 (products below 2^43); it depends on the edge
//             alone, so two faces that share an edge agree: rows are watertight.  Edge-on faces cover nothing.
//   position  n = (b - a) x (c - a) in int64; in fp64, in this order, uncontracted: num = n.y (p.y - a.y) + n.z (p.z - a.z),
//             x = a.x - num / n.x, i0 = clamp(ceil(x / 64), 0, W).  The crossing toggles every cell i >= i0 of the row.
//   fill      a cell is inside iff the number of toggles at or before it is odd; a row whose parity at index W is odd is open.
//
// Two launches over a workspace of one toggle bit per (k, j, i0), i0 in 0..W, zeroed on the caller's stream by the entry point:
//   voxel_faces_kernel  XORs a bit per crossing with vector global atomics.  XOR commutes: the bits do not depend on arrival order.
//   voxel_fill_kernel   one wave per row turns the toggle bits into prefix parities and stores the inside cells.
// Compiled with -ffp-contract=off (the position above is the model's only with separate multiplies and adds).
#include "../../include/fluidnet_hip.h"
#include "fnx_cells.h"
#include "fnx_device.h"
#include "fnx_kernels.h"
#include <algorithm>

namespace {

// ---- primitives ---------------------------------------------------------------------------------------------------------------------
// Sphere: createCylinder's arithmetic with a third term -- float(i) - cx, squared, summed x, y, z in that order, compared with
// float(r * r): the slice k == cz of a sphere is the cylinder's disc bit for bit (dz * dz = +0).  Box: half open like createBox2D.
// blockIdx.z walks nb * D plane slices of the samples [b0, b0 + nb).
template <bool BOX>
__global__ __launch_bounds__(BX* BY) void geometry3d_kernel(GridDims g, float* __restrict__ flags, int b0, float a0, float a1, float a2,
                                                            float a3, float a4, float a5) {
  const CellId c = cell_id<true>(g);
  if (!c.valid) return;
  bool inside;
  const float x = (float)c.i, y = (float)c.j, z = (float)c.k;
  if (BOX) {
    inside = (x >= a0) & (x < a1) & (y >= a2) & (y < a3) & (z >= a4) & (z < a5);
  } else {
    const float dx = x - a0, dy = y - a1, dz = z - a2;
    inside = dx * dx + dy * dy + dz * dz <= a3;
  }
  if (inside) flags[(size_t)(b0 + c.b) * g.DHW + (size_t)c.k * g.HW + c.j * g.W + c.i] = FNX_OBST;
}

// ---- the face pass ------------------------------------------------------------------------------------------------------------------
constexpr int SNAP = 64;                    // sub-cell lattice of the snapped vertices
constexpr long long QMAX = 1ll << 20;       // |q| above this: a bad face
constexpr int SOLO_POINTS = 8;              // a face whose (y, z) box holds at most this many rows is walked by its own lane

// floor and ceiling of q / 64 for any sign
__device__ __forceinline__ int floor64(int q) { return q >> 6; }
__device__ __forceinline__ int ceil64(int q) { return (q + (SNAP - 1)) >> 6; }

struct Face {
  int ax, ay, az, bx, by, bz, cx, cy, cz;   // snapped vertices (|q| <= 2^20)
  int jlo, klo, nj, nk;                     // the rows its (y, z) box can cover, clipped to the grid: nj * nk of them (0: none)
};

// snaps vertex `idx` of face f; false: bad
__device__ __forceinline__ bool snap_vertex(const float* __restrict__ vertices, int n_vertices, int idx, int& qx, int& qy, int& qz) {
  if (idx < 0 || idx >= n_vertices) return false;
  const float* v = vertices + (size_t)idx * 3;
  const double x = (double)v[0] * (double)SNAP, y = (double)v[1] * (double)SNAP, z = (double)v[2] * (double)SNAP;
  // NaN fails every comparison; Inf and far vertices fail the bound (before any conversion to an integer)
  if (!(fabs(x) <= (double)QMAX + 1.0) || !(fabs(y) <= (double)QMAX + 1.0) || !(fabs(z) <= (double)QMAX + 1.0)) return false;
  const long long lx = (long long)rint(x), ly = (long long)rint(y), lz = (long long)rint(z);
  if (lx > QMAX || lx < -QMAX || ly > QMAX || ly < -QMAX || lz > QMAX || lz < -QMAX) return false;
  qx = (int)lx; qy = (int)ly; qz = (int)lz;
  return true;
}

__device__ __forceinline__ bool edge_crossed(int ay, int az, int by, int bz, long long py, long long pz) {
  if (((long long)az > pz) == ((long long)bz > pz)) return false;
  if (az > bz) { int t = ay; ay = by; by = t; t = az; az = bz; bz = t; }
  const long long s = (long long)(by - ay) * (pz - (long long)az) - (py - (long long)ay) * (long long)(bz - az);
  return s > 0;
}

// row (j, k) against face F: toggles the row's bit at the crossing, if the face covers the row
__device__ __forceinline__ void face_row(const Face& F, int j, int k, const GridDims& g, int wpr, unsigned* __restrict__ bits) {
  const long long py = (long long)j * SNAP, pz = (long long)k * SNAP;
  const bool cover = edge_crossed(F.ay, F.az, F.by, F.bz, py, pz) ^ edge_crossed(F.by, F.bz, F.cy, F.cz, py, pz) ^
                     edge_crossed(F.cy, F.cz, F.ay, F.az, py, pz);
  if (!cover) return;
  const long long ux = F.bx - F.ax, uy = F.by - F.ay, uz = F.bz - F.az, vx = F.cx - F.ax, vy = F.cy - F.ay, vz = F.cz - F.az;
  const long long nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
  if (nx == 0) return;                                     // cannot be (an edge-on face covers nothing); keeps the division finite
  const double num = (double)ny * (double)(py - F.ay) + (double)nz * (double)(pz - F.az);
  const double x = (double)F.ax - num / (double)nx;
  const double c = ceil(x * (1.0 / SNAP));
  const int i0 = !(c > 0.0) ? 0 : (c >= (double)g.W ? g.W : (int)c);
  atomicXor(bits + ((size_t)k * g.H + j) * wpr + (i0 >> 5), 1u << (i0 & 31));
}

// A lane takes a face.  Small faces (sub-cell meshes: most cover one row or none) are walked by their lanes at once.  The wave then
// takes its lanes' large faces one at a time -- found by a ballot, handed over by lane reads -- with the rows of the face's box spread
// over the lanes, so that two faces spanning the domain do not serialise on two lanes.  gridDim.y parts share the rows of the large
// faces (a mesh of few faces fills the chip that way; the launcher gives a mesh of many faces one part); part 0 alone walks the small
// faces and counts the bad ones.
__global__ __launch_bounds__(256) void voxel_faces_kernel(GridDims g, int wpr, const float* __restrict__ vertices, int n_vertices,
                                                          const int* __restrict__ faces, int n_faces, unsigned* __restrict__ bits,
                                                          int* __restrict__ counters) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int part = blockIdx.y, parts = gridDim.y;
  Face F;
  F.nj = F.nk = 0; F.jlo = F.klo = 0;
  F.ax = F.ay = F.az = F.bx = F.by = F.bz = F.cx = F.cy = F.cz = 0;
  if (f < n_faces) {
    const int* idx = faces + (size_t)f * 3;
    const bool oka = snap_vertex(vertices, n_vertices, idx[0], F.ax, F.ay, F.az);
    const bool okb = snap_vertex(vertices, n_vertices, idx[1], F.bx, F.by, F.bz);
    const bool okc = snap_vertex(vertices, n_vertices, idx[2], F.cx, F.cy, F.cz);
    if (oka && okb && okc) {
      const int ymin = min(F.ay, min(F.by, F.cy)), ymax = max(F.ay, max(F.by, F.cy));
      const int zmin = min(F.az, min(F.bz, F.cz)), zmax = max(F.az, max(F.bz, F.cz));
      // a crossed edge has min z <= p.z < max z; the y box is the triangle's
      const int jlo = max(ceil64(ymin), 0), jhi = min(floor64(ymax), g.H - 1);
      const int klo = max(ceil64(zmin), 0), khi = min(ceil64(zmax) - 1, g.D - 1);
      if (jhi >= jlo && khi >= klo) { F.jlo = jlo; F.klo = klo; F.nj = jhi - jlo + 1; F.nk = khi - klo + 1; }
    } else if (part == 0) {
      atomicAdd(counters + 1, 1);
    }
  }
  const int npts = F.nj * F.nk;                           // <= D * H < 2^31
  const bool solo = npts <= SOLO_POINTS;
  if (solo && part == 0) {
    for (int t = 0; t < npts; ++t) face_row(F, F.jlo + t % F.nj, F.klo + t / F.nj, g, wpr, bits);
  }
  unsigned long long big = __ballot(!solo);
  while (big) {
    const int src = __ffsll((long long)big) - 1;
    big &= big - 1;
    Face S;
    S.ax = __shfl(F.ax, src); S.ay = __shfl(F.ay, src); S.az = __shfl(F.az, src);
    S.bx = __shfl(F.bx, src); S.by = __shfl(F.by, src); S.bz = __shfl(F.bz, src);
    S.cx = __shfl(F.cx, src); S.cy = __shfl(F.cy, src); S.cz = __shfl(F.cz, src);
    S.jlo = __shfl(F.jlo, src); S.klo = __shfl(F.klo, src); S.nj = __shfl(F.nj, src); S.nk = __shfl(F.nk, src);
    const int n = S.nj * S.nk;                            // <= D * H < 2^31 / 3: t + parts * 64 cannot wrap
    for (int t = part * 64 + lane; t < n; t += parts * 64) {
      const int kk = t / S.nj;
      face_row(S, S.jlo + (t - kk * S.nj), S.klo + kk, g, wpr, bits);
    }
  }
}

// ---- the fill pass ------------------------------------------------------------------------------------------------------------------
// One wave per row (k, j), a lane per 32-bit word, 64 words (2048 cells) at a time.  A word's prefix parities come from shifts; the
// carry into a word is the parity of the lower lanes' words (a ballot of word parities, masked) and of the chunks before, handed on
// in a register.  A chunk without a toggle and without a carry is left at once.  The stores go to inside cells only, 64 consecutive
// cells per wave instruction: lane l takes bit (l & 31) of word 2 s + (l >> 5) of the chunk from its owner.
__global__ __launch_bounds__(256) void voxel_fill_kernel(GridDims g, int wpr, int b0, int nb, const unsigned* __restrict__ bits,
                                                         float* __restrict__ flags, int* __restrict__ counters) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);     // k * H + j
  if (row >= g.D * g.H) return;                            // wave-uniform
  const int lane = threadIdx.x & 63;
  const unsigned* rbits = bits + (size_t)row * wpr;
  unsigned carry = 0;                                      // parity of every toggle before this chunk
  for (int w0 = 0; w0 < wpr; w0 += 64) {
    const int w = w0 + lane;
    unsigned x = w < wpr ? rbits[w] : 0u;
    const unsigned long long any = __ballot(x != 0u);
    if (any == 0ull && carry == 0u) continue;
    const unsigned long long odd = __ballot((__popc(x) & 1) != 0);
    x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16;     // bit t: parity of the bits 0..t
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    if ((carry ^ (unsigned)__popcll(odd & below)) & 1u) x = ~x;
    carry ^= (unsigned)__popcll(odd) & 1u;
    const unsigned long long inside = __ballot(x != 0u);
    for (int s = 0; s < 32; ++s) {
      if (((inside >> (2 * s)) & 3ull) == 0ull) continue;   // wave-uniform
      const unsigned word = __shfl(x, 2 * s + (lane >> 5));
      const int i = (w0 + 2 * s) * 32 + lane;
      if (i < g.W && ((word >> (lane & 31)) & 1u)) {
        for (int b = b0; b < b0 + nb; ++b) flags[(size_t)b * g.DHW + (size_t)row * g.W + i] = FNX_OBST;
      }
    }
  }
  // bit W lives in the row's last word and no bit lies beyond it: the parity at index W is the carry out of the row
  if (lane == 0 && carry) atomicAdd(counters, 1);
}

}  // namespace

namespace fnx {

void launch_create_sphere(const GridDims& g, float* flags, int b0, int nb, float cx, float cy, float cz, float r2, hipStream_t s) {
  GridDims d = g; d.B = nb;
  geometry3d_kernel<false><<<cell_grid(d), dim3(BX, BY), 0, s>>>(g, flags, b0, cx, cy, cz, r2, 0.f, 0.f);
}

void launch_create_box3d(const GridDims& g, float* flags, int b0, int nb, float x0, float x1, float y0, float y1, float z0, float z1,
                         hipStream_t s) {
  GridDims d = g; d.B = nb;
  geometry3d_kernel<true><<<cell_grid(d), dim3(BX, BY), 0, s>>>(g, flags, b0, x0, x1, y0, y1, z0, z1);
}

void launch_voxelize_mesh(const GridDims& g, float* flags, int b0, int nb, const float* vertices, int n_vertices, const int* faces,
                          int n_faces, unsigned* bits, int* counters, hipStream_t s) {
  const int wpr = voxel_words_per_row(g);
  if (n_faces > 0) {
    const unsigned blocks = (unsigned)(((long long)n_faces + 255) / 256);
    // parts: enough waves for the chip when the mesh has few faces (which are then large), one part for a mesh of many
    const long long waves = (long long)blocks * 4;
    const int parts = (int)std::max(1ll, std::min(64ll, 2048 / waves));
    voxel_faces_kernel<<<dim3(blocks, parts), 256, 0, s>>>(g, wpr, vertices, n_vertices, faces, n_faces, bits, counters);
  }
  const unsigned rows = (unsigned)g.D * (unsigned)g.H;
  voxel_fill_kernel<<<(rows + 3) / 4, 256, 0, s>>>(g, wpr, b0, nb, bits, flags, counters);
}

}  // namespace fnx
