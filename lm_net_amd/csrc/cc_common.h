// The connected-component core under the 2D cleaning (postprocess.hip) and the 3D cleaning (volpost.hip): the tile geometry, the
// union-find in LDS and in the global parent array with the argument for its safety, the tile and the seam pass of one image or one
// slice, the in-place root walk, the pre-reduced per-wave count and the selection key.  Device helpers only, no kernels: the
// __global__ kernels keep their names in their own files and call these.
//
// INDEX SPACE.  Every helper works in an index space in which an element of row y and column x of the plane at hand has the index
// base + y * W + x, and every pointer it takes is indexed by that.  The 2D cleaning passes pointers offset by the image and base 0
// (an image pixel index); the 3D cleaning passes the volume's pointers and the slice offset as base (a volume voxel index).  Either
// way a parent is always the smaller index, a tile root is the smallest index of its tile component -- within one plane the index
// orders elements as the tile-local index does row by row, and base is common -- and a component's root ends up as its smallest
// index.  All indices are below 2^30 + 1023 (sides <= 1024) and therefore int32.
#pragma once
#include "common.h"

#define CC_TH 32
#define CC_TW 64
#define CC_PPT (CC_TH * CC_TW / 256)            // elements per thread of the tile pass, consecutive in a row
#define CC_SEGS (CC_TW / CC_PPT)                // threads per tile row

namespace {

// a label as a pass reads it.  CLAMP: values >= C are 0 (C = 256: every value stands); otherwise the map holds clamped labels already
template <bool CLAMP>
__device__ __forceinline__ int cc_lab(const uint8_t* __restrict__ L, int i, int C) {
  const int l = L[i];
  return !CLAMP || l < C ? l : 0;
}

// ---------------------------------------------------------------- union-find in LDS (tile-local indices)
__device__ __forceinline__ int cc_tile_find(int* par, int i) {
  int r = i;
  for (;;) {
    const int p = __hip_atomic_load(par + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == r) break;
    r = p;
  }
  return r;
}
// Lock-free union: the larger root takes the smaller as its parent.  Every iteration either ends or lowers a parent.  (atomicMin
// also re-points an `a` that is no root any more; the loop then unites a's old parent with b, and with no path compression in
// cc_tile_find nothing can drop that duty -- unlike in the global union-find below.)
__device__ __forceinline__ void cc_tile_union(int* par, int a, int b) {
  for (;;) {
    a = cc_tile_find(par, a);
    b = cc_tile_find(par, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(par + a, b);
    if (old == a) return;
    a = old;                                                 // a was no root any more: go on from what it pointed to
  }
}

// ---------------------------------------------------------------- union-find in the global parent array
// SAFETY, for an index space in which a tile root is the smallest index of its tile component (above).  The per-XCD L2s are not
// coherent with each other, so a load of a parent (relaxed, agent scope: it bypasses the L1 only) may return an OLD value.  That is
// safe.  The invariant: every value a node's parent ever had is a member of the node's current TREE with an index <= the node's,
// at every later moment, and parents only ever decrease.  (Not "an ancestor": the path compression below re-points a node past its
// old parent.)  The tile pass establishes it.  A link changes the pointer of a node that IS a root at that moment and of no other
// (the compare-and-swap below), so it merges two whole trees and no tree ever loses a member.  So a walk over old values strictly
// descends inside one tree and ends, after at most as many steps as the tree has members, at a node that was a root at some time.
// Whether it still IS one the atomic alone decides: atomicCAS(parent[a], a, b) returns the node's true parent at that moment; when
// that is the node itself the link has been made, otherwise NOTHING was written and the loop goes on from the returned value, which
// is smaller.  Equal roots of both ends prove one tree.  Path compression writes min(parent, r) with r < n a member of n's tree: n
// moves with its subtree to another place of the same tree, and the parent it leaves keeps its own pointer, so the tree stays
// whole; it never changes a current root, because a root is the smallest index of its tree (the loop runs while n > r).
// The link must NOT be an atomicMin(parent[a], b): that also re-points an `a` that is no root any more, into b's tree, and hands the
// caller the duty to unite a's old parent with b.  Until that is done the trees are not the sets, and a compression that started
// from an old value of a subtree node may pull a's ancestors out of the chain that leads to the owed link: the link is then lost
// (found by replaying random interleavings; seen on the device as one root too many in about one 3D labelling in fifty).
// NO KERNEL WAITS FOR ANOTHER BLOCK: there is no lock, no grid barrier and no "retry until someone else has written"; every loop
// either lowers a parent, descends to a smaller node or ends, and an index is bounded below by 0.
__device__ __forceinline__ int cc_find(int32_t* par, int i) {
  int r = i, steps = 0;
  for (;;) {
    const int p = __hip_atomic_load(par + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == r) break;
    r = p;                                                   // p < r: the walk descends
    ++steps;
  }
  if (steps > 1) {                                           // compress the walked path: r is in the set of each of its nodes
    int n = i;
    while (n > r) n = atomicMin(par + n, r);                 // n strictly decreases: the walk left n for a smaller parent, and parents only decrease
  }
  return r;
}
__device__ __forceinline__ void cc_union(int32_t* par, int a, int b) {
  for (;;) {
    a = cc_find(par, a);                                     // the finds come first: two ends of one set issue no atomic
    b = cc_find(par, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicCAS(par + a, a, b);                // links a only while a is a root (the argument above)
    if (old == a) return;
    a = old;                                                 // a was no root any more: go on from its parent, old < a
  }
}

// ---------------------------------------------------------------- the tile pass of one plane
// One 256-thread block labels the CC_TH x CC_TW tile (blockIdx.x, blockIdx.y) inside LDS (2 KiB of labels + 8 KiB of tile-local
// parents) and writes, for every element, the tile root of its component as an index of the index space.
// only_zero: the hole labelling -- elements of a non-zero label join nothing (they stay their own roots and are not counted)
template <bool CLAMP>
__device__ __forceinline__ void cc_tile_body(const uint8_t* __restrict__ L, int32_t* __restrict__ P, int base, int H, int W, int C,
                                             int conn8, int only_zero) {
  __shared__ uint8_t s_lab[CC_TH * CC_TW];
  __shared__ int s_par[CC_TH * CC_TW];
  const int tx0 = blockIdx.x * CC_TW, ty0 = blockIdx.y * CC_TH;
  const int twv = min(CC_TW, W - tx0), thv = min(CC_TH, H - ty0);          // the tile's valid extent
  const int row = threadIdx.x / CC_SEGS, x0 = (threadIdx.x % CC_SEGS) * CC_PPT;
  const int t0 = row * CC_TW + x0;                                         // tile-local index of the thread's first element
  const int g0 = base + (ty0 + row) * W + tx0 + x0;                        // ... and its index
  const bool rowv = row < thv;
  const int nv = rowv ? max(0, min(CC_PPT, twv - x0)) : 0;                 // valid elements of this thread
#pragma unroll
  for (int j = 0; j < CC_PPT; ++j) s_lab[t0 + j] = j < nv ? (uint8_t)cc_lab<CLAMP>(L, g0 + j, C) : (uint8_t)0;
  __syncthreads();
  // row runs: an element points at the first element of its run inside the thread's segment, a segment's first element at its left
  // neighbour
  {
    int start = t0;
    for (int j = 0; j < nv; ++j) {
      const int i = t0 + j;
      const uint8_t l = s_lab[i];
      const bool joins = !(only_zero && l != 0);
      const bool cont = joins && (j > 0 || x0 > 0) && s_lab[i - 1] == l;     // the run goes on from the left neighbour
      if (j == 0 || !cont) start = i;
      s_par[i] = !cont ? i : (j == 0 ? i - 1 : start);
    }
  }
  __syncthreads();
  // Unions with the row above.  An edge is skipped when a neighbour's edge implies it: the vertical edge when the left element and
  // the upper-left element both have the label (the left element's vertical edge joins the same two runs); a diagonal edge when the
  // element above has the label (it lies in the diagonal element's run), when the left element has it (upper-left: its vertical
  // edge) or the right element has it (upper-right: its vertical edge).
  if (row > 0) {
    for (int j = 0; j < nv; ++j) {
      const int i = t0 + j, x = x0 + j;
      const uint8_t l = s_lab[i];
      if (only_zero && l != 0) continue;
      const bool left = x > 0 && s_lab[i - 1] == l;
      if (s_lab[i - CC_TW] == l) {
        if (!(left && s_lab[i - CC_TW - 1] == l)) cc_tile_union(s_par, i, i - CC_TW);
      } else if (conn8) {
        if (x > 0 && !left && s_lab[i - CC_TW - 1] == l) cc_tile_union(s_par, i, i - CC_TW - 1);
        if (x + 1 < twv && s_lab[i + 1] != l && s_lab[i - CC_TW + 1] == l) cc_tile_union(s_par, i, i - CC_TW + 1);
      }
    }
  }
  __syncthreads();
  for (int j = 0; j < nv; ++j) {
    const int r = cc_tile_find(s_par, t0 + j);
    P[g0 + j] = base + (ty0 + r / CC_TW) * W + tx0 + r % CC_TW;
  }
}

// ---------------------------------------------------------------- the seam pass of one plane
// One thread (number blockIdx.x * 256 + threadIdx.x) per element below a horizontal seam (rows y = k * CC_TH) and right of a vertical
// seam (columns x = k * CC_TW): the edges to its in-plane neighbours on the other side, united in the global parent array.  A corner
// element's edges are issued twice, which is harmless.
template <bool CLAMP>
__device__ __forceinline__ void cc_seam_body(const uint8_t* __restrict__ L, int32_t* P, int base, int H, int W, int C, int conn8,
                                             int only_zero) {
  const int nhs = (H - 1) / CC_TH, nvs = (W - 1) / CC_TW;                // seams inside the plane
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < nhs * W) {
    const int s = idx / W, x = idx - s * W, y = (s + 1) * CC_TH;
    const int i = base + y * W + x;
    const int l = cc_lab<CLAMP>(L, i, C);
    if (only_zero && l != 0) return;
    if (cc_lab<CLAMP>(L, i - W, C) == l) {
      cc_union(P, i, i - W);
    } else if (conn8) {
      if (x > 0 && cc_lab<CLAMP>(L, i - W - 1, C) == l) cc_union(P, i, i - W - 1);
      if (x + 1 < W && cc_lab<CLAMP>(L, i - W + 1, C) == l) cc_union(P, i, i - W + 1);
    }
  } else if (idx < nhs * W + nvs * H) {
    const int k = idx - nhs * W;
    const int s = k / H, y = k - s * H, x = (s + 1) * CC_TW;
    const int i = base + y * W + x;
    const int l = cc_lab<CLAMP>(L, i, C);
    if (only_zero && l != 0) return;
    if (cc_lab<CLAMP>(L, i - 1, C) == l) {
      cc_union(P, i, i - 1);
    } else if (conn8) {                                    // (with the left element in the set its vertical edges imply both diagonals;
      if (y > 0 && cc_lab<CLAMP>(L, i - W - 1, C) == l) cc_union(P, i, i - W - 1);       //  the element below, if in the set, issues the lower one itself)
      if (y + 1 < H && cc_lab<CLAMP>(L, i + W - 1, C) == l && cc_lab<CLAMP>(L, i + W, C) != l) cc_union(P, i, i + W - 1);
    }
  }
}

// ---------------------------------------------------------------- flatten: the root walk and the count
// Walk to the root of i and store it at i, in place: an element's final root is a member of its set with a smaller index, so a
// concurrent walk that reads the old or the new value still descends inside the set; no union runs beside a flatten pass, so a root
// read as a root is one.
__device__ __forceinline__ int cc_root_store(int32_t* par, int i) {
  int r = i;
  for (;;) {
    const int p = __hip_atomic_load(par + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == r) break;
    r = p;
  }
  __hip_atomic_store(par + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return r;
}

// dst[key] += 1 for every lane with `counted`, pre-reduced per wave: the wave's first four distinct keys add their lane counts once;
// whatever is left adds 1 per lane (exact either way).  dst is global memory or LDS.  EVERY lane of the wave must reach this call
// (the ballots), counted or not.
__device__ __forceinline__ void cc_wave_count(bool counted, int key, int* dst) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(counted);
  for (int it = 0; it < 4 && todo; ++it) {
    const int leader = __ffsll((long long)todo) - 1;
    const int k0 = __shfl(key, leader, 64);
    const unsigned long long same = __ballot(key == k0) & todo;               // (todo holds counted lanes only)
    if (lane == leader) atomicAdd(dst + k0, __popcll(same));
    todo &= ~same;
  }
  if ((todo >> lane) & 1) atomicAdd(dst + key, 1);
}

// ---------------------------------------------------------------- the selection key
// A 64-bit atomic max over (size << 32) | ~root settles "largest size, then smallest root" by itself; 0 is no component.
typedef unsigned long long cc_u64;
__device__ __forceinline__ cc_u64 cc_key(int size, int root) { return ((cc_u64)(uint32_t)size << 32) | (0xFFFFFFFFu - (uint32_t)root); }
__device__ __forceinline__ int cc_key_size(cc_u64 key) { return (int)(key >> 32); }
__device__ __forceinline__ int cc_key_root(cc_u64 key) { return (int)(0xFFFFFFFFu - (uint32_t)key); }

}  // namespace
