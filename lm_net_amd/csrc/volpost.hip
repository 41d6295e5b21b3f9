// 3D connected-component cleaning of a label volume on the device (lm_net_amd.post.VolumePostprocess; include/volpost/
// lmnet_volpost.h): the components of a [D, H, W] uint8 volume under connectivity 6, 18 or 26, the n largest of a class (n <= 4),
// a minimal volume, cavity filling under the dual connectivity, per-class statistics.  postprocess.hip with one more axis: the same
// tile and seam passes and the same union-find (cc_common.h: LDS tiles per slice, lock-free unions, and the argument for
// their safety), a volume-sized index space, links to the slice above and a selection of several components.  Integer arithmetic
// throughout; every cross-block sum is an int32 atomic add, every selection a 64-bit atomic max and every mark an atomic or, so the
// result does not depend on arrival order: two calls give bit-identical outputs.
//
// Labelling (lmn_cc3d_label, and twice inside lmn_volpost_clean), every label value partitioned:
//   1. vp_tile_kernel     one 256-thread block labels a 32 x 64 tile of ONE slice inside LDS (2 KiB of labels + 8 KiB of tile-local
//                         parents): row runs, then unions with the row above -- 4-connected in the plane for 6, 8-connected for 18
//                         and 26 -- then every voxel writes the tile root of its component as a VOLUME voxel index.
//   2. vp_seam_kernel     one thread per voxel next to an in-plane tile seam unites the trees across the seam.
//   3. vp_zlink_kernel    one thread per voxel of the slices z >= 1 unites it with the voxels of equal label among the up to 9 voxels
//                         of slice z - 1 that the connectivity allows (1 for 6, 5 for 18, 9 for 26).  This is the new cost: one
//                         candidate set per voxel and not per seam voxel, so the links that the plane labellings of the two slices
//                         imply are cut first (vp_zlink_kernel's comment), and a find on both ends precedes any atomic.
//   4. vp_flatten_kernel  every voxel finds its root (in place) and adds 1 to sizes[root] (pre-reduced per wave); for the hole
//                         labelling a voxel on one of the six faces sets its root's bit in a bitmap of its own (a size reaches 2^30:
//                         the size word has no room for a mark).
//
// INDEX WIDTH.  D, H, W <= 1024, so a voxel index (z * H + y) * W + x < 2^30 and a size <= 2^30 are int32, and so are the block
// arithmetic of every kernel here (at most 2^30 + 1023).  A byte offset into the int32 arrays is not: every pointer is formed as
// `base + index` on a typed pointer, which the compiler widens to 64 bits.
//
// SAFETY of the union-find in the global parent array: the comment at cc_find (cc_common.h).  Its index space here is the volume
// voxel index: the tile and the seam pass take the volume's pointers and the slice offset as base, and vp_zlink_kernel's links keep
// the invariant as every union does (the smaller root becomes the parent).
//
// Cleaning (lmn_volpost_clean):
//   5. vp_select_kernel   pass j = 0 .. max(keep_largest) - 1: root voxels offer (size << 32 | ~root) to slot (class, j), restricted
//                         for j >= 1 to keys below slot (class, j - 1): block-level max in LDS, then one 64-bit atomic max per
//                         block and slot.  The packed key (cc_common.h) settles "largest size, then smallest root".  Pass 0 counts the components.
//   6. vp_apply_kernel    L1 = L0 without the components that do not survive keep_largest / min_volume.
//   7. (labelling of L1's zero voxels under the dual connectivity with face marks) vp_fill_kernel: holes take the label at x - 1 of
//      their root voxel; per-class voxel counts and the number of holes.
#include "cc_common.h"
#include "../../include/volpost/lmnet_volpost.h"

#define VP_MAXSIDE LMN_VOLPOST_MAX_SIDE
#define VP_MAXKEEP LMN_VOLPOST_MAX_KEEP
#define VP_PPB 1024                           // voxels per block of the select and fill passes

namespace {

typedef unsigned long long vp_u64;

struct VpParam {
  uint64_t class_mask;
  int32_t min_volume[64];
  uint8_t keep[64];                           // 0 = every component, else the number of largest components kept
};

inline int64_t vp_face_bytes(int64_t V) { return lmn_up256(4 * ((V + 31) / 32)); }

// a label as the cleaning reads it: values >= C are 0 (C = 256: every value stands)
__device__ __forceinline__ int vp_lab(const uint8_t* __restrict__ L, int i, int C) { return cc_lab<true>(L, i, C); }

// The tile and the seam pass of slice blockIdx.z / blockIdx.y (cc_common.h), in volume voxel indices: the slice's first voxel (< 2^30)
// is the base.  only_zero: the hole labelling -- voxels of a non-zero label join nothing (they stay their own roots and are not counted)
__global__ __launch_bounds__(256) void vp_tile_kernel(const uint8_t* __restrict__ lab, int H, int W, int C, int conn8, int only_zero,
                                                      int32_t* __restrict__ parent) {
  cc_tile_body<true>(lab, parent, (int)blockIdx.z * H * W, H, W, C, conn8, only_zero);
}

__global__ __launch_bounds__(256) void vp_seam_kernel(const uint8_t* __restrict__ lab, int H, int W, int C, int conn8, int only_zero,
                                                      int32_t* parent) {
  cc_seam_body<true>(lab, parent, (int)blockIdx.y * H * W, H, W, C, conn8, only_zero);
}

// Links to the slice above.  v = (z, y, x) with label l; its candidates are the voxels u = (z - 1, y + dy, x + dx) of label l with
// (dy, dx) allowed by the connectivity: (0, 0) for 6; dy == 0 or dx == 0 for 18; all nine for 26.  Slice z - 1 is labelled in the plane
// (4-connected for 6, 8-connected for 18 and 26), and so is slice z, which makes most candidates redundant.  A link is cut when the
// other links and the plane labellings join the same two sets:
//   (a) the centre (0, 0) has the label: every other candidate is its in-plane neighbour (a row or column neighbour under 18, any of
//       the eight under 26), so the centre link alone is issued;
//   (b) otherwise a candidate (dy, +-1) whose row neighbour (dy, 0) is a candidate too is that one's run mate: cut;
//   (c) v continues a row run, i.e. w = (z, y, x - 1) has the label (v and w are one set).  Then u is cut when w links to it itself,
//       (dy, dx + 1) being allowed, or when u's left neighbour has the label: w links to that voxel, (dy, dx) being allowed, and it
//       is u's run mate.  So inside a run only the first voxel tests all its upper neighbours; the others test what the new column
//       brings: nothing under 6 while the upper run goes on, the column x + 1 under 26, (0, +1) and (+-1, 0) under 18.
// By induction along the run every allowed link of w is issued or implied, so (c) loses nothing; (a) and (b) replace a link by an
// in-plane path.  allow: bit 3 * (dy + 1) + (dx + 1).
__global__ __launch_bounds__(256) void vp_zlink_kernel(const uint8_t* __restrict__ lab, int H, int W, int C, int allow, int only_zero,
                                                       int total, int32_t* parent) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;                                              // total = (D - 1) * H * W
  const int HW = H * W;
  const int i = t + HW;                                                // the voxel: slices 1 .. D - 1
  const int l = vp_lab(lab, i, C);
  if (only_zero && l != 0) return;
  const int yx = t % HW, y = yx / W, x = yx - y * W;
  const int up = i - HW;
  const bool run = x > 0 && vp_lab(lab, i - 1, C) == l;               // v continues a row run
  if (vp_lab(lab, up, C) == l) {                                       // (a)
    if (!(run && vp_lab(lab, up - 1, C) == l)) cc_union(parent, i, up);   // (c): x > 0, so up - 1 is in the row
    return;
  }
  if (allow == (1 << 4)) return;                                       // connectivity 6: the centre was the only candidate
  for (int dy = -1; dy <= 1; ++dy) {
    if (y + dy < 0 || y + dy >= H) continue;
    const int rowc = up + dy * W;                                      // (z - 1, y + dy, x)
    const bool mid = dy != 0 && vp_lab(lab, rowc, C) == l;             // (dy, 0) is a candidate ((0, 0) is not: handled above)
    for (int dx = -1; dx <= 1; ++dx) {
      if (!((allow >> (3 * (dy + 1) + dx + 1)) & 1) || (dy == 0 && dx == 0)) continue;
      if (x + dx < 0 || x + dx >= W) continue;
      if (dx != 0 && mid) continue;                                    // (b)
      const int u = rowc + dx;
      if (dx == 0 ? !mid : vp_lab(lab, u, C) != l) continue;
      if (run) {                                                       // (c)
        if (dx <= 0 && ((allow >> (3 * (dy + 1) + dx + 2)) & 1)) continue;
        if (x + dx > 0 && vp_lab(lab, u - 1, C) == l) continue;
      }
      cc_union(parent, i, u);
    }
  }
}

__global__ __launch_bounds__(256) void vp_flatten_kernel(const uint8_t* __restrict__ lab, int D, int H, int W, int C, int only_zero,
                                                         int V, int32_t* roots, int32_t* __restrict__ sizes, uint32_t* __restrict__ face) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool counted = false;
  int r = -1;
  if (i < V && !(only_zero && vp_lab(lab, i, C) != 0)) {
    counted = true;
    r = cc_root_store(roots, i);
    if (face) {
      const int HW = H * W, z = i / HW, yx = i - z * HW, y = yx / W, x = yx - y * W;
      if (z == 0 || z == D - 1 || y == 0 || y == H - 1 || x == 0 || x == W - 1) atomicOr(face + (r >> 5), 1u << (r & 31));
    }
  }
  cc_wave_count(counted, r, sizes);
}

// Pass `rank` of the selection.  best[k * VP_MAXKEEP + j]: the key of class k's (j + 1)-th largest component, 0 = there is none.
// A block reduces its offers per class in LDS first, so a volume in which every voxel is a root (the parity checkerboard under 6)
// still issues one global atomic per block and class.
__global__ __launch_bounds__(256) void vp_select_kernel(const uint8_t* __restrict__ lab, const int32_t* __restrict__ roots,
                                                        const int32_t* __restrict__ sizes, int V, int C, VpParam prm, int rank,
                                                        vp_u64* best, int32_t* __restrict__ stats) {
  __shared__ vp_u64 s_best[64], s_below[64];
  __shared__ int s_n[64], s_pass[64];
  if (threadIdx.x < 64) {
    const int k = threadIdx.x;
    s_best[k] = 0;
    s_n[k] = 0;
    s_pass[k] = 0;
    // keys of this pass lie below the previous rank's (written by the previous launch); no previous component: nothing is offered
    s_below[k] = rank == 0 ? ~0ull : best[k * VP_MAXKEEP + rank - 1];
  }
  __syncthreads();
  for (int it = 0; it < VP_PPB / 256; ++it) {
    const int i = blockIdx.x * VP_PPB + it * 256 + threadIdx.x;
    if (i < V && roots[i] == i) {
      const int k = vp_lab(lab, i, C), a = sizes[i];
      if (rank == 0) atomicAdd(&s_n[k], 1);
      if (prm.keep[k] > rank) {
        const vp_u64 key = cc_key(a, i);
        if (key < s_below[k]) atomicMax(&s_best[k], key);
      } else if (rank == 0 && prm.keep[k] == 0 && (!((prm.class_mask >> k) & 1) || a >= prm.min_volume[k])) {
        atomicAdd(&s_pass[k], 1);
      }
    }
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < C) {
    if (s_n[k]) atomicAdd(stats + k * 4, s_n[k]);
    if (s_pass[k]) atomicAdd(stats + k * 4 + 1, s_pass[k]);
    if (s_best[k]) atomicMax(best + k * VP_MAXKEEP + rank, s_best[k]);
  }
}

__global__ __launch_bounds__(256) void vp_apply_kernel(const uint8_t* __restrict__ lab, const int32_t* __restrict__ roots,
                                                       const int32_t* __restrict__ sizes, int V, int C, VpParam prm,
                                                       const vp_u64* __restrict__ best, uint8_t* __restrict__ out,
                                                       int32_t* __restrict__ stats) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < C && prm.keep[threadIdx.x]) {          // survivors of a keep_largest class
    const int k = threadIdx.x;
    int n = 0;
    for (int j = 0; j < prm.keep[k]; ++j) {
      const vp_u64 w = best[k * VP_MAXKEEP + j];
      n += (w != 0 && cc_key_size(w) >= prm.min_volume[k]) ? 1 : 0;
    }
    stats[k * 4 + 1] = n;
  }
  if (i >= V) return;
  int k = vp_lab(lab, i, C);
  if ((prm.class_mask >> k) & 1) {
    const int r = roots[i];
    bool keep = sizes[r] >= prm.min_volume[k];
    if (prm.keep[k]) {
      bool among = false;
      for (int j = 0; j < prm.keep[k]; ++j) {
        const vp_u64 w = best[k * VP_MAXKEEP + j];
        among = among || (w != 0 && cc_key_root(w) == r);
      }
      keep = keep && among;
    }
    if (!keep) k = 0;
  }
  out[i] = (uint8_t)k;
}

// lab = L1 (values < C).  roots / sizes / face: the labelling of lab's zero voxels under the dual connectivity, or NULL (no filling)
__global__ __launch_bounds__(256) void vp_fill_kernel(const uint8_t* __restrict__ lab, const int32_t* __restrict__ roots,
                                                      const int32_t* __restrict__ sizes, const uint32_t* __restrict__ face, int V, int C,
                                                      int hole_limit, uint8_t* __restrict__ out, int32_t* __restrict__ stats) {
  __shared__ int s_cnt[64];
  __shared__ int s_holes;
  if (threadIdx.x < 64) s_cnt[threadIdx.x] = 0;
  if (threadIdx.x == 0) s_holes = 0;
  __syncthreads();
  for (int it = 0; it < VP_PPB / 256; ++it) {                   // (a uniform trip count: every lane reaches cc_wave_count's ballots)
    const int i = blockIdx.x * VP_PPB + it * 256 + threadIdx.x;
    int k = -1;
    if (i < V) {
      k = lab[i];
      if (roots && k == 0) {
        const int r = roots[i];
        if (!((face[r >> 5] >> (r & 31)) & 1) && sizes[r] <= hole_limit) {
          k = lab[r - 1];                      // x - 1 of the root: inside the volume (the hole touches no face), not 0
          if (r == i) atomicAdd(&s_holes, 1);
        }
      }
      out[i] = (uint8_t)k;
    }
    cc_wave_count(k >= 0, k, s_cnt);
  }
  __syncthreads();
  if (threadIdx.x < C && s_cnt[threadIdx.x]) atomicAdd(stats + threadIdx.x * 4 + 2, s_cnt[threadIdx.x]);
  if (threadIdx.x == 0 && s_holes) atomicAdd(stats + 3, s_holes);
}

bool vp_dims_ok(int D, int H, int W) {
  return D >= 1 && D <= VP_MAXSIDE && H >= 2 && H <= VP_MAXSIDE && W >= 2 && W <= VP_MAXSIDE;
}

// the candidate offsets of a connectivity, bit 3 * (dy + 1) + (dx + 1)
int vp_allow(int connectivity) { return connectivity == 6 ? 0x010 : connectivity == 18 ? 0x0BA : 0x1FF; }

// the four labelling kernels on zeroed `sizes` (and `face`, where given)
void vp_label(const uint8_t* lab, int D, int H, int W, int C, int connectivity, int only_zero, int32_t* roots, int32_t* sizes,
              uint32_t* face, hipStream_t st) {
  const int conn8 = connectivity != 6;
  const int V = D * H * W, nseam = ((H - 1) / CC_TH) * W + ((W - 1) / CC_TW) * H, nz = (D - 1) * H * W;
  LMN_LAUNCH(vp_tile_kernel, dim3(lmn_cdiv(W, CC_TW), lmn_cdiv(H, CC_TH), D), dim3(256), 0, st, lab, H, W, C, conn8, only_zero, roots);
  if (nseam > 0) LMN_LAUNCH(vp_seam_kernel, dim3(lmn_cdiv(nseam, 256), D), dim3(256), 0, st, lab, H, W, C, conn8, only_zero, roots);
  if (nz > 0) LMN_LAUNCH(vp_zlink_kernel, dim3(lmn_cdiv(nz, 256)), dim3(256), 0, st, lab, H, W, C, vp_allow(connectivity), only_zero, nz, roots);
  LMN_LAUNCH(vp_flatten_kernel, dim3(lmn_cdiv(V, 256)), dim3(256), 0, st, lab, D, H, W, C, only_zero, V, roots, sizes, face);
}

}  // namespace

extern "C" {

int64_t lmn_volpost_workspace(int D, int H, int W) {
  if (!vp_dims_ok(D, H, W)) {
    snprintf(g_lmn_err, sizeof(g_lmn_err), "volpost_workspace: D=%d %dx%d outside D in [1, %d], sides in [2, %d]", D, H, W, VP_MAXSIDE,
             VP_MAXSIDE);
    return -1;
  }
  const int64_t V = (int64_t)D * H * W;
  return lmn_up256(V) + 2 * lmn_up256(4 * V) + vp_face_bytes(V) + lmn_up256(64 * VP_MAXKEEP * 8);
}

int lmn_cc3d_label(const uint8_t* labels, int D, int H, int W, int connectivity, int32_t* roots, int32_t* sizes, lmn_stream_t stream) {
  LMN_REQUIRE(labels && roots && sizes, "cc3d_label: null pointer");
  LMN_REQUIRE(D >= 1 && D <= VP_MAXSIDE, "cc3d_label: D=%d not in [1, %d]", D, VP_MAXSIDE);
  LMN_REQUIRE(H >= 2 && H <= VP_MAXSIDE && W >= 2 && W <= VP_MAXSIDE, "cc3d_label: size %dx%d outside [2, %d]", H, W, VP_MAXSIDE);
  LMN_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, "cc3d_label: connectivity %d is none of 6, 18, 26", connectivity);
  hipStream_t st = (hipStream_t)stream;
  LMN_HIP_OK(hipMemsetAsync(sizes, 0, sizeof(int32_t) * (size_t)D * H * W, st), "cc3d_label");
  vp_label(labels, D, H, W, 256, connectivity, 0, roots, sizes, nullptr, st);
  return lmn_launch_status("cc3d_label");
}

int lmn_volpost_clean(const uint8_t* labels, int D, int H, int W, int C, int connectivity, uint64_t class_mask,
                      const int32_t* keep_largest, const int32_t* min_volume, int hole_limit, void* workspace, int64_t ws_bytes,
                      uint8_t* labels_out, int32_t* stats, lmn_stream_t stream) {
  LMN_REQUIRE(labels && keep_largest && min_volume && workspace && labels_out && stats, "volpost_clean: null pointer");
  LMN_REQUIRE(C >= 2 && C <= 64, "volpost_clean: C=%d not in [2, 64]", C);
  LMN_REQUIRE(D >= 1 && D <= VP_MAXSIDE, "volpost_clean: D=%d not in [1, %d]", D, VP_MAXSIDE);
  LMN_REQUIRE(H >= 2 && H <= VP_MAXSIDE && W >= 2 && W <= VP_MAXSIDE, "volpost_clean: size %dx%d outside [2, %d]", H, W, VP_MAXSIDE);
  LMN_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, "volpost_clean: connectivity %d is none of 6, 18, 26",
              connectivity);
  const uint64_t all = C == 64 ? ~0ull : ((1ull << C) - 1);
  LMN_REQUIRE(!(class_mask & 1) && !(class_mask & ~all), "volpost_clean: class_mask names class 0 or a class >= C=%d", C);
  LMN_REQUIRE(hole_limit >= 0, "volpost_clean: hole_limit %d < 0", hole_limit);
  VpParam prm;
  memset(&prm, 0, sizeof(prm));
  prm.class_mask = class_mask;
  int ranks = 0;
  for (int k = 0; k < C; ++k) {
    LMN_REQUIRE(keep_largest[k] >= 0 && keep_largest[k] <= VP_MAXKEEP, "volpost_clean: keep_largest[%d] = %d outside [0, %d]", k,
                (int)keep_largest[k], VP_MAXKEEP);
    LMN_REQUIRE(keep_largest[k] == 0 || ((class_mask >> k) & 1), "volpost_clean: keep_largest[%d] = %d names a class outside class_mask", k,
                (int)keep_largest[k]);
    LMN_REQUIRE(min_volume[k] >= 0, "volpost_clean: min_volume[%d] = %d < 0", k, (int)min_volume[k]);
    prm.keep[k] = (uint8_t)keep_largest[k];
    prm.min_volume[k] = ((class_mask >> k) & 1) ? min_volume[k] : 0;
    if (keep_largest[k] > ranks) ranks = keep_largest[k];
  }
  const int64_t need = lmn_volpost_workspace(D, H, W);
  LMN_REQUIRE(ws_bytes >= need, "volpost_clean: workspace of %lld bytes too small, %lld needed", (long long)ws_bytes, (long long)need);
  const int64_t V64 = (int64_t)D * H * W;
  const int V = (int)V64;
  uint8_t* lab1 = (uint8_t*)workspace;
  int32_t* roots = (int32_t*)(lab1 + lmn_up256(V64));
  int32_t* sizes = (int32_t*)((uint8_t*)roots + lmn_up256(4 * V64));
  uint32_t* face = (uint32_t*)((uint8_t*)sizes + lmn_up256(4 * V64));
  vp_u64* best = (vp_u64*)((uint8_t*)face + vp_face_bytes(V64));
  hipStream_t st = (hipStream_t)stream;
  const dim3 pgrid(lmn_cdiv(V, 256)), wgrid(lmn_cdiv(V, VP_PPB));
  LMN_HIP_OK(hipMemsetAsync(stats, 0, sizeof(int32_t) * 4 * (size_t)C, st), "volpost_clean");
  LMN_HIP_OK(hipMemsetAsync(sizes, 0, (size_t)(need - lmn_up256(V64) - lmn_up256(4 * V64)), st), "volpost_clean");     // sizes, face and best, adjacent
  vp_label(labels, D, H, W, C, connectivity, 0, roots, sizes, nullptr, st);
  for (int rank = 0; rank < (ranks > 1 ? ranks : 1); ++rank)
    LMN_LAUNCH(vp_select_kernel, wgrid, dim3(256), 0, st, labels, (const int32_t*)roots, (const int32_t*)sizes, V, C, prm, rank, best, stats);
  LMN_LAUNCH(vp_apply_kernel, pgrid, dim3(256), 0, st, labels, (const int32_t*)roots, (const int32_t*)sizes, V, C, prm, (const vp_u64*)best,
             lab1, stats);
  const int32_t* hroots = nullptr;
  if (hole_limit > 0) {
    LMN_HIP_OK(hipMemsetAsync(sizes, 0, sizeof(int32_t) * (size_t)V, st), "volpost_clean");
    vp_label(lab1, D, H, W, C, connectivity == 6 ? 26 : 6, 1, roots, sizes, face, st);                  // the dual connectivity
    hroots = roots;
  }
  LMN_LAUNCH(vp_fill_kernel, wgrid, dim3(256), 0, st, (const uint8_t*)lab1, hroots, (const int32_t*)sizes, (const uint32_t*)face, V, C,
             hole_limit, labels_out, stats);
  return lmn_launch_status("volpost_clean");
}

}  // extern "C"
