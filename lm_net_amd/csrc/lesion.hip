// Per-lesion matching of a predicted and a target label volume on the device (lm_net_amd.metrics.LesionMeter; include/lesion/
// lmnet_lesion.h): the components of both volumes (lmn_cc3d_label of volpost.hip, called as it stands), one record per lesion of a
// scored class, and the JOIN of the two labellings -- for every pair of a predicted and a target lesion of one class that share a
// voxel, the number of shared voxels.  Integer arithmetic and integer atomics only.
//
//   ls_match_kernel   one 256-thread block per LS_PPB = 1024 consecutive voxels, four consecutive voxels per lane (one 4-byte load
//                     from each label volume, one 16-byte load from each roots and sizes array where the pointers allow; a scalar
//                     path covers the last voxels and unaligned pointers).
//     components      a root voxel has sizes > 0.  Root voxels of scored classes append (side << 40 | class << 32 | root, size):
//                     eight ballots (two sides x four voxels), ONE atomic add per wave on ctrl[0], records beyond the capacity are
//                     counted and not written.
//     pairs           a voxel whose two labels agree on a scored class carries the key root_p << 32 | root_g.  Per voxel slot the
//                     wave's first two distinct keys are counted by ballot and inserted once by their first lane; the other lanes
//                     insert their own.  An insertion goes into the block's table in LDS (LS_LDS slots, linear probing over at most
//                     LS_LDS_PROBES of them: 64-bit compare-and-swap on the key, add on the count); when that finds no slot, the
//                     insertion goes straight into the global table.  After a barrier every occupied LDS slot does ONE global
//                     insertion, so two full masks cost one global compare-and-swap per block and not one per voxel.
//
// THE GLOBAL TABLE.  pair_slots (a power of two) keys of 64 bits, EMPTY = all bits set (no key: roots are below 2^30), and as many
// int32 counts, both set by the entry before the launch.  An insertion of (key, n) probes linearly from hash(key): atomicCAS(slot,
// EMPTY, key) returns EMPTY (the slot is now this key's) or key (it was already) -- add n to the slot's count and stop -- or
// another key: go on to the next slot.  Only the value the compare-and-swap returns decides whose slot it is: there is no plain
// load of a table word, so the per-XCD L2s cannot show a stale one (device-scope atomics are performed where all XCDs meet; the
// SAFETY comment at cc_find in cc_common.h).  A key is never removed and a slot never changes its key, so a key sits in at most one
// slot: the first slot from hash(key) that ever held it, every earlier slot of the probe sequence having been taken by other keys
// before.  TERMINATION: the probe loop runs over at most pair_slots slots (LS_LDS_PROBES in LDS) and then gives up -- the insertion
// is counted in ctrl[2] and dropped.  NO KERNEL WAITS FOR ANOTHER THREAD OR BLOCK: no lock, no spin, no "retry until someone else has
// written".  Which slot a record lands in, and which insertion a full table drops, depend on arrival order; with ctrl[2] == 0 the
// SET of records does not, since the counts are integer sums.
#include "common.h"
#include "../../include/lesion/lmnet_lesion.h"
#include "../../include/volpost/lmnet_volpost.h"

#define LS_MAXSIDE LMN_LESION_MAX_SIDE
#define LS_PPB 1024                           // voxels per block (VP_PPB of volpost.hip)
#define LS_LDS 256                            // slots of the block's table in LDS (3 KiB)
#define LS_LDS_PROBES 16                      // ... and the slots one insertion tries there before it goes to the global table
#define LS_EMPTY (~0ull)

namespace {

typedef unsigned long long ls_u64;

__device__ __forceinline__ uint32_t ls_hash(uint32_t rp, uint32_t rg) { return lmn_hash32(rp ^ lmn_hash32(rg + 0x9E3779B9u)); }

// (key, n) into the global table: 1 = a new slot, 0 = added to the key's slot, -1 = no slot in `slots` probes (nothing written)
__device__ __forceinline__ int ls_global_insert(ls_u64* keys, int32_t* counts, int slots, ls_u64 key, uint32_t h, int n) {
  uint32_t s = h & (uint32_t)(slots - 1);
  for (int probe = 0; probe < slots; ++probe) {
    const ls_u64 old = atomicCAS(keys + s, LS_EMPTY, key);
    if (old == LS_EMPTY || old == key) {
      atomicAdd(counts + s, n);
      return old == LS_EMPTY ? 1 : 0;
    }
    s = (s + 1) & (uint32_t)(slots - 1);
  }
  return -1;
}

// (key, n) into the block's table; false = no slot among LS_LDS_PROBES (nothing written).  (Other hash bits than the global table's.)
__device__ __forceinline__ bool ls_lds_insert(ls_u64* s_key, int* s_cnt, ls_u64 key, uint32_t h, int n) {
  uint32_t s = (h >> 22) & (LS_LDS - 1);
  for (int probe = 0; probe < LS_LDS_PROBES; ++probe) {
    const ls_u64 old = atomicCAS(s_key + s, LS_EMPTY, key);
    if (old == LS_EMPTY || old == key) {
      atomicAdd(s_cnt + s, n);
      return true;
    }
    s = (s + 1) & (LS_LDS - 1);
  }
  return false;
}

struct LsTable {
  ls_u64* keys;
  int32_t* counts;
  int slots;
};

// one insertion of the pair pass: the block's table, else the global one; s_stat[0] / [1] count new global slots / full-table drops
__device__ __forceinline__ void ls_insert(ls_u64* s_key, int* s_cnt, int* s_stat, LsTable t, int rp, int rg, int n) {
  const ls_u64 key = ((ls_u64)(uint32_t)rp << 32) | (uint32_t)rg;
  const uint32_t h = ls_hash((uint32_t)rp, (uint32_t)rg);
  if (ls_lds_insert(s_key, s_cnt, key, h, n)) return;
  const int r = ls_global_insert(t.keys, t.counts, t.slots, key, h, n);
  if (r != 0) atomicAdd(s_stat + (r > 0 ? 0 : 1), 1);
}

__global__ __launch_bounds__(256) void ls_match_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ target,
                                                       const int32_t* __restrict__ roots_p, const int32_t* __restrict__ sizes_p,
                                                       const int32_t* __restrict__ roots_g, const int32_t* __restrict__ sizes_g, int V, int C,
                                                       uint64_t class_mask, int vec, ls_u64* __restrict__ comp_keys,
                                                       int32_t* __restrict__ comp_sizes, int max_components, LsTable table, int32_t* ctrl) {
  __shared__ ls_u64 s_key[LS_LDS];
  __shared__ int s_cnt[LS_LDS];
  __shared__ int s_stat[2];
  for (int s = threadIdx.x; s < LS_LDS; s += 256) {
    s_key[s] = LS_EMPTY;
    s_cnt[s] = 0;
  }
  if (threadIdx.x < 2) s_stat[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int i0 = blockIdx.x * LS_PPB + threadIdx.x * 4;                // <= 2^30 + 1020: an int32
  // lab[side][j], root[side][j], size[side][j] of the lane's four voxels; a voxel past the volume is background with size 0
  int lab[2][4], root[2][4], size[2][4];
  if (vec && i0 + 3 < V) {
    const uint32_t a = *reinterpret_cast<const uint32_t*>(pred + i0), b = *reinterpret_cast<const uint32_t*>(target + i0);
    const int4 rp = *reinterpret_cast<const int4*>(roots_p + i0), rg = *reinterpret_cast<const int4*>(roots_g + i0);
    const int4 sp = *reinterpret_cast<const int4*>(sizes_p + i0), sg = *reinterpret_cast<const int4*>(sizes_g + i0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      lab[0][j] = (a >> (8 * j)) & 0xFF;
      lab[1][j] = (b >> (8 * j)) & 0xFF;
    }
    root[0][0] = rp.x; root[0][1] = rp.y; root[0][2] = rp.z; root[0][3] = rp.w;
    root[1][0] = rg.x; root[1][1] = rg.y; root[1][2] = rg.z; root[1][3] = rg.w;
    size[0][0] = sp.x; size[0][1] = sp.y; size[0][2] = sp.z; size[0][3] = sp.w;
    size[1][0] = sg.x; size[1][1] = sg.y; size[1][2] = sg.z; size[1][3] = sg.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool in = i0 + j < V;
      lab[0][j] = in ? pred[i0 + j] : 0;
      lab[1][j] = in ? target[i0 + j] : 0;
      root[0][j] = in ? roots_p[i0 + j] : 0;
      root[1][j] = in ? roots_g[i0 + j] : 0;
      size[0][j] = in ? sizes_p[i0 + j] : 0;
      size[1][j] = in ? sizes_g[i0 + j] : 0;
    }
  }
  bool scored[2][4];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int l = lab[q >> 2][q & 3] < C ? lab[q >> 2][q & 3] : 0;     // a value >= C is background (C <= 64: the shift is in range)
    lab[q >> 2][q & 3] = l;
    scored[q >> 2][q & 3] = (class_mask >> l) & 1;
  }
  // ---- the component records.  Every lane of the wave reaches the ballots.
  {
    unsigned long long bal[8];
    int total = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      bal[q] = __ballot(scored[q >> 2][q & 3] && size[q >> 2][q & 3] > 0);
      total += __popcll(bal[q]);
    }
    if (total) {                                                       // (wave-uniform)
      int base = 0;
      if (lane == 0) base = atomicAdd(ctrl, total);
      base = __shfl(base, 0, 64);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        if ((bal[q] >> lane) & 1) {
          const int idx = base + __popcll(bal[q] & ((1ull << lane) - 1));
          if (idx < max_components) {
            const int side = q >> 2, j = q & 3;
            comp_keys[idx] = ((ls_u64)side << 40) | ((ls_u64)lab[side][j] << 32) | (uint32_t)(i0 + j);
            comp_sizes[idx] = size[side][j];
          }
        }
        base += __popcll(bal[q]);
      }
    }
  }
  // ---- the pairs: per voxel slot the wave's first two distinct keys go in once, with the number of their lanes
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool v = scored[0][j] && lab[0][j] == lab[1][j];
    const int rp = root[0][j], rg = root[1][j];
    unsigned long long todo = __ballot(v);
    for (int it = 0; it < 2 && todo; ++it) {                           // (todo is wave-uniform)
      const int leader = __ffsll((long long)todo) - 1;
      const int p0 = __shfl(rp, leader, 64), g0 = __shfl(rg, leader, 64);
      const unsigned long long same = __ballot(v && rp == p0 && rg == g0) & todo;
      if (lane == leader) ls_insert(s_key, s_cnt, s_stat, table, p0, g0, __popcll(same));
      todo &= ~same;
    }
    if ((todo >> lane) & 1) ls_insert(s_key, s_cnt, s_stat, table, rp, rg, 1);
  }
  __syncthreads();
  // ---- one global insertion per occupied slot of the block's table
  for (int s = threadIdx.x; s < LS_LDS; s += 256) {
    const ls_u64 key = s_key[s];
    if (key != LS_EMPTY) {
      const int r = ls_global_insert(table.keys, table.counts, table.slots, key, ls_hash((uint32_t)(key >> 32), (uint32_t)key), s_cnt[s]);
      if (r != 0) atomicAdd(s_stat + (r > 0 ? 0 : 1), 1);
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 && s_stat[threadIdx.x]) atomicAdd(ctrl + 1 + threadIdx.x, s_stat[threadIdx.x]);
}

bool ls_dims_ok(int D, int H, int W) {
  return D >= 1 && D <= LS_MAXSIDE && H >= 2 && H <= LS_MAXSIDE && W >= 2 && W <= LS_MAXSIDE;
}

}  // namespace

extern "C" {

int64_t lmn_lesion_workspace(int D, int H, int W) {
  if (!ls_dims_ok(D, H, W)) {
    snprintf(g_lmn_err, sizeof(g_lmn_err), "lesion_workspace: D=%d %dx%d outside D in [1, %d], sides in [2, %d]", D, H, W, LS_MAXSIDE,
             LS_MAXSIDE);
    return -1;
  }
  return 4 * lmn_up256(4 * (int64_t)D * H * W);
}

int lmn_lesion_match(const uint8_t* pred, const uint8_t* target, int D, int H, int W, int C, int connectivity, uint64_t class_mask,
                     void* workspace, int64_t ws_bytes, int64_t* comp_keys, int32_t* comp_sizes, int max_components, int64_t* pair_keys,
                     int32_t* pair_counts, int pair_slots, int32_t* ctrl, lmn_stream_t stream) {
  LMN_REQUIRE(pred && target && workspace && comp_keys && comp_sizes && pair_keys && pair_counts && ctrl, "lesion_match: null pointer");
  LMN_REQUIRE(C >= 2 && C <= 64, "lesion_match: C=%d not in [2, 64]", C);
  LMN_REQUIRE(D >= 1 && D <= LS_MAXSIDE, "lesion_match: D=%d not in [1, %d]", D, LS_MAXSIDE);
  LMN_REQUIRE(H >= 2 && H <= LS_MAXSIDE && W >= 2 && W <= LS_MAXSIDE, "lesion_match: size %dx%d outside [2, %d]", H, W, LS_MAXSIDE);
  LMN_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, "lesion_match: connectivity %d is none of 6, 18, 26",
              connectivity);
  const uint64_t all = C == 64 ? ~0ull : ((1ull << C) - 1);
  LMN_REQUIRE(!(class_mask & 1) && !(class_mask & ~all), "lesion_match: class_mask names class 0 or a class >= C=%d", C);
  LMN_REQUIRE(pair_slots >= LMN_LESION_MIN_SLOTS && pair_slots <= LMN_LESION_MAX_SLOTS && !(pair_slots & (pair_slots - 1)),
              "lesion_match: pair_slots %d is no power of two in [%d, %d]", pair_slots, LMN_LESION_MIN_SLOTS, LMN_LESION_MAX_SLOTS);
  LMN_REQUIRE(max_components >= 1, "lesion_match: max_components %d < 1", max_components);
  const int64_t need = lmn_lesion_workspace(D, H, W);
  LMN_REQUIRE(ws_bytes >= need, "lesion_match: workspace of %lld bytes too small, %lld needed", (long long)ws_bytes, (long long)need);
  const int64_t V64 = (int64_t)D * H * W, part = lmn_up256(4 * V64);
  const int V = (int)V64;
  int32_t* roots_p = (int32_t*)workspace;
  int32_t* sizes_p = (int32_t*)((uint8_t*)workspace + part);
  int32_t* roots_g = (int32_t*)((uint8_t*)workspace + 2 * part);
  int32_t* sizes_g = (int32_t*)((uint8_t*)workspace + 3 * part);
  hipStream_t st = (hipStream_t)stream;
  LMN_HIP_OK(hipMemsetAsync(comp_keys, 0xFF, sizeof(int64_t) * (size_t)max_components, st), "lesion_match");
  LMN_HIP_OK(hipMemsetAsync(comp_sizes, 0, sizeof(int32_t) * (size_t)max_components, st), "lesion_match");
  LMN_HIP_OK(hipMemsetAsync(pair_keys, 0xFF, sizeof(int64_t) * (size_t)pair_slots, st), "lesion_match");
  LMN_HIP_OK(hipMemsetAsync(pair_counts, 0, sizeof(int32_t) * (size_t)pair_slots, st), "lesion_match");
  LMN_HIP_OK(hipMemsetAsync(ctrl, 0, sizeof(int32_t) * LMN_LESION_NCTRL, st), "lesion_match");
  int rc = lmn_cc3d_label(pred, D, H, W, connectivity, roots_p, sizes_p, stream);
  if (rc != 0) return rc;
  rc = lmn_cc3d_label(target, D, H, W, connectivity, roots_g, sizes_g, stream);
  if (rc != 0) return rc;
  // the vector loads: 4 bytes of each label volume, 16 bytes of each workspace array (the arrays start 256-byte multiples apart)
  const int vec = (((uintptr_t)pred | (uintptr_t)target) & 3) == 0 && ((uintptr_t)workspace & 15) == 0;
  const LsTable table = {(ls_u64*)pair_keys, pair_counts, pair_slots};
  LMN_LAUNCH(ls_match_kernel, dim3(lmn_cdiv(V, LS_PPB)), dim3(256), 0, st, pred, target, (const int32_t*)roots_p, (const int32_t*)sizes_p,
             (const int32_t*)roots_g, (const int32_t*)sizes_g, V, C, class_mask, vec, (ls_u64*)comp_keys, comp_sizes, max_components, table,
             ctrl);
  return lmn_launch_status("lesion_match");
}

}  // extern "C"
