// Context shift (ops.kv_shift): move KV rows between blocks of the paged cache and re-rotate the keys.
//
// The cache stores K already rotated by RoPE, so a token that moves from position p to p - delta needs its K row
// rotated by -delta; V does not depend on the position.  The arena is kv [L, 2, NB, Hkv, 64, 128] bf16.  A move is
// (src, dst, row_lo, row_hi, delta): in every layer and KV head, for rows row_lo <= r < row_hi,
//   K row r of dst = K row r of src rotated by -delta   (delta 0: a plain copy)
//   V row r of dst = V row r of src                     (src == dst: V is not touched at all)
// Rotate-half convention (norm_rope.hip, ops/reference.py rope_append): the pair is (i, i + 64), and with
// c = cos[delta][i], s = sin[delta][i] from the model's own f32 tables
//   lo' = lo * c + hi * s,   hi' = hi * c - lo * s
// computed in f32 from the stored bf16 with every product and sum rounded on its own (no fused multiply-add, so the
// host twin's torch arithmetic gives the same bits), then rounded once to nearest-even bf16.
//
// grid (move, layer, 2 * Hkv * 2), 256 threads: a workgroup takes 32 rows of one (K | V, head) tile, a lane the two
// 16-byte pieces that hold dims 8j .. 8j+7 and 64+8j .. 64+8j+7 of one row -- both halves of its 8 pairs, so an
// in-place move has no hazard between lanes and needs no LDS.  Every lane issues its loads (two pieces, and for K
// the 8 cos and 8 sin values) before its stores; every K / V byte is read once and written at most once.  Plain
// 16-byte vector loads and stores only.  The host refuses move lists in which a destination row range overlaps
// another destination or another move's source (ops.kv_shift), so no workgroup reads a word that another one
// writes.  A move with an id outside (0, NB), rows outside 0 <= lo <= hi <= 64 or a delta outside the tables is
// skipped here, as kv_copy_blocks_kernel skips a bad pair.
#include "common.h"

constexpr int KVS_THREADS = 256, KVS_ROWS = KVS_THREADS / 8;

// A product as its own rounded f32: the empty asm makes the value opaque, so the build's -ffp-contract=fast (which
// ignores a contract(off) pragma) cannot fuse it into the sum that follows as v_fma / v_pk_fma.
__device__ __forceinline__ float kvs_rounded(float v) {
  asm("" : "+v"(v));
  return v;
}

__global__ __launch_bounds__(KVS_THREADS) void kv_shift_kernel(uint4* kv, const int* __restrict__ moves, int nb,
                                                               int hkv, const float4* __restrict__ cos_t,
                                                               const float4* __restrict__ sin_t, int table_rows) {
  const int* mv = moves + 5 * blockIdx.x;
  const int src = mv[0], dst = mv[1], lo = mv[2], hi = mv[3], delta = mv[4];
  if (src <= 0 || src >= nb || dst <= 0 || dst >= nb || lo < 0 || hi > 64 || lo > hi || delta < 0 ||
      delta >= table_rows)
    return;
  const int z = blockIdx.z, half = z & 1, h = (z >> 1) % hkv, is_v = (z >> 1) / hkv;
  if (src == dst && (is_v || delta == 0)) return;  // nothing moves
  const int row = half * KVS_ROWS + (threadIdx.x >> 3), j = threadIdx.x & 7;
  if (row < lo || row >= hi) return;
  const size_t plane = ((size_t)blockIdx.y * 2 + is_v) * nb;
  const size_t in_tile = ((size_t)h * 64 + row) * 16 + j;  // 16-byte units: a row is 16 of them
  const uint4* ps = kv + (plane + src) * (size_t)hkv * 1024 + in_tile;
  uint4* pd = kv + (plane + dst) * (size_t)hkv * 1024 + in_tile;
  const uint4 a = ps[0], b = ps[8];
  if (is_v || delta == 0) {
    pd[0] = a;
    pd[8] = b;
    return;
  }
  const float4* pc = cos_t + (size_t)delta * 16 + 2 * j;  // a table row is 64 f32 = 16 float4
  const float4* pn = sin_t + (size_t)delta * 16 + 2 * j;
  const float4 c0 = pc[0], c1 = pc[1], s0 = pn[0], s1 = pn[1];
  const float c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
  const float s[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
  float x[8], y[8], xo[8], yo[8];
  unpack8(a, x);
  unpack8(b, y);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    xo[i] = kvs_rounded(x[i] * c[i]) + kvs_rounded(y[i] * s[i]);
    yo[i] = kvs_rounded(y[i] * c[i]) - kvs_rounded(x[i] * s[i]);
  }
  pd[0] = pack8(xo);
  pd[8] = pack8(yo);
}

// kv: the [L, 2, NB, Hkv, 64, 128] bf16 arena; moves: device int32 [n, 5]; cos / sin: f32 [table_rows, 64]
extern "C" int lsa_kv_shift(void* kv, const int* moves, int n, int layers, int nb, int hkv, const float* cos_t,
                            const float* sin_t, int table_rows, hipStream_t s) {
  if (n <= 0) return 0;
  if (layers <= 0 || layers > 65535 || n > 65535 || nb < 2 || hkv <= 0 || 4 * hkv > 65535 || table_rows <= 0 ||
      kv == nullptr || moves == nullptr || cos_t == nullptr || sin_t == nullptr)
    return -1;
  hipLaunchKernelGGL(kv_shift_kernel, dim3(n, layers, 4 * hkv), dim3(KVS_THREADS), 0, s, reinterpret_cast<uint4*>(kv),
                     moves, nb, hkv, reinterpret_cast<const float4*>(cos_t), reinterpret_cast<const float4*>(sin_t),
                     table_rows);
  return (int)hipGetLastError();
}
