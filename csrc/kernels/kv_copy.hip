// Paged-KV block copy (prefix cache, ops.kv_copy_blocks): fork a partly matching cached block.
//
// The arena is kv [L, 2, NB, Hkv, 64, 128] (bf16, or e4m3 bytes with scales [L, 2, NB, Hkv, 64] f32), so the
// [Hkv, 64, 128] tile of one block in one (layer, K|V) plane is one contiguous run: 512 KiB on the 7B, 128 KiB on
// the 3B, 8 KiB for one fp8 head.  For every pair (src, dst) the tile of src, and its scale tile, is copied to dst
// in every plane.  The whole block is copied: rows at or past the matched length are stale, and the prefill that
// follows overwrites them before anything reads them (every attention kernel bounds its reads by the context).
//
// grid (pair, 2 L, chunks), 256 threads: a workgroup moves KVC_UNITS 16-byte units of the run "tile, then scale
// tile" of its plane, KVC_UNROLL per lane, loads first and stores after.  One launch covers every pair, and a
// single 7B block is 56 x 32 workgroups.  Plain loads and stores: the prefill that follows reads the copy, and
// other sharers may be reading the source.  The last chunk is guarded (the run is no multiple of KVC_UNITS for
// small tiles and for every fp8 tile).  Block ids are checked on the host; a pair outside (0, NB) is skipped here.
#include "common.h"

constexpr int KVC_THREADS = 256, KVC_UNROLL = 4, KVC_UNITS = KVC_THREADS * KVC_UNROLL;

__global__ __launch_bounds__(KVC_THREADS) void kv_copy_blocks_kernel(uint4* kv, uint4* sc,
                                                                     const int* __restrict__ pairs, int nb,
                                                                     int tile_units, int scale_units) {
  const int src = pairs[2 * blockIdx.x], dst = pairs[2 * blockIdx.x + 1];
  if (src <= 0 || src >= nb || dst <= 0 || dst >= nb || src == dst) return;
  const size_t plane = (size_t)blockIdx.y * nb;
  const uint4* ks = kv + (plane + src) * (size_t)tile_units;
  uint4* kd = kv + (plane + dst) * (size_t)tile_units;
  const uint4* ss = sc + (plane + src) * (size_t)scale_units;  // never read when scale_units == 0
  uint4* sd = sc + (plane + dst) * (size_t)scale_units;
  const int total = tile_units + scale_units;
  const int u0 = blockIdx.z * KVC_UNITS + threadIdx.x;
  uint4 v[KVC_UNROLL];
#pragma unroll
  for (int i = 0; i < KVC_UNROLL; ++i) {
    const int u = u0 + i * KVC_THREADS;
    if (u < tile_units) v[i] = ks[u];
    else if (u < total) v[i] = ss[u - tile_units];
  }
#pragma unroll
  for (int i = 0; i < KVC_UNROLL; ++i) {
    const int u = u0 + i * KVC_THREADS;
    if (u < tile_units) kd[u] = v[i];
    else if (u < total) sd[u - tile_units] = v[i];
  }
}

// tile_bytes / scale_bytes: bytes of one block in one plane (multiples of 16; scale_bytes 0 for the bf16 cache)
extern "C" int lsa_kv_copy_blocks(void* kv, void* scale, const int* pairs, int npairs, int planes, int nb,
                                  long long tile_bytes, long long scale_bytes, hipStream_t s) {
  if (npairs <= 0) return 0;
  if (planes <= 0 || planes > 65535 || npairs > 65535 || nb < 2 || tile_bytes <= 0 || tile_bytes % 16 ||
      scale_bytes < 0 || scale_bytes % 16 || (scale_bytes > 0 && scale == nullptr))
    return -1;
  const long long units = (tile_bytes + scale_bytes) / 16;
  const long long chunks = (units + KVC_UNITS - 1) / KVC_UNITS;
  if (chunks > 65535) return -2;
  hipLaunchKernelGGL(kv_copy_blocks_kernel, dim3(npairs, planes, (unsigned)chunks), dim3(KVC_THREADS), 0, s,
                     reinterpret_cast<uint4*>(kv), reinterpret_cast<uint4*>(scale), pairs, nb, (int)(tile_bytes / 16),
                     (int)(scale_bytes / 16));
  return (int)hipGetLastError();
}
