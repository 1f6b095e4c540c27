// Chamfer distance between two clouds a (B,N,3) and bp (B,M,3): the self-supervised loss's
// nearest-neighbour term (selfsup.py).  No reference counterpart in this model family's CUDA
// extension: PointPWC-Net's loss builds it from a dense (B,N,M) distance matrix in torch.
//
// Forward, one launch for both directions (blockIdx.z = 0: every row of a against bp;
// blockIdx.z = 1: every row of bp against a):
//
//   dist[q] = min_r dist3(ref[r], qry[q]),  idx[q] = the lowest r that attains it
//
// dist3 is the direct-difference form (kdpc_common.h), so the distance of a point to itself is
// exactly 0 wherever the clouds lie; the comparison is strict < in ascending r, so the lower
// index wins ties: the first column of kdpc_three_nn, bit for bit.  The running best starts at
// (+inf, 0) and a NaN distance passes no test, so idx is always in range.
//
// Scan: flow_propagate.hip's.  One thread per query; the reference cloud staged through LDS in
// 1024-point tiles (12 KiB) and read back as broadcasts, 8 points (6 x 16 bytes) at a time,
// their 8 distances formed before one test of their minimum against the running best.  Writes
// dist / idx only: no workspace, no atomics, no allocation.
//
// Backward, for one cloud (the other one's is the same entry with the roles swapped):
//
//   da[i] = 2 g_ab[i] (a_i - bp[idx_ab[i]]) + sum_{j : idx_ba[j] = i} 2 g_ba[j] (a_i - bp_j)
//
// one thread per row of a; the sum runs over the row's run of the CSR of idx_ba (kdpc_csr_build,
// ascending j) after the direct term, each term entering through one fma: a fixed order, no
// atomics.
#include "kdpc_common.h"

using namespace kdpc;

namespace {

constexpr int kChTile = 1024;  // reference points per LDS tile (flow_propagate.hip's kFpTile)
constexpr int kChBlock = 256;
constexpr int kChChunk = 8;  // reference points whose distances are formed together
static_assert(kChTile % kChChunk == 0 && (kChChunk * 3) % 4 == 0, "chunks are whole float4s");

__global__ __launch_bounds__(kChBlock) void chamfer_fwd_kernel(
    int n, int m, const float* __restrict__ a, const float* __restrict__ bp,
    float* __restrict__ dist_ab, int* __restrict__ idx_ab, float* __restrict__ dist_ba,
    int* __restrict__ idx_ba) {
  __shared__ float4 sk4[kChTile * 3 / 4];
  float* sk = reinterpret_cast<float*>(sk4);
  const bool ba = blockIdx.z != 0;  // direction: block-uniform
  const int nq = ba ? m : n, nr = ba ? n : m;
  const int first = blockIdx.x * kChBlock;
  if (first >= nq) return;  // block-uniform: before any barrier
  const int bi = blockIdx.y;
  const float* qry = (ba ? bp : a) + (long long)bi * nq * 3;
  const float* ref = (ba ? a : bp) + (long long)bi * nr * 3;
  const int row = first + threadIdx.x;
  const bool active = row < nq;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (active) {
    qx = qry[(long long)row * 3 + 0];
    qy = qry[(long long)row * 3 + 1];
    qz = qry[(long long)row * 3 + 2];
  }
  float best = INFINITY;
  int ibest = 0;
  for (int t0 = 0; t0 < nr; t0 += kChTile) {
    const int tn = min(kChTile, nr - t0);
    const int tpad = divup(tn, kChChunk) * kChChunk;  // <= kChTile
    __syncthreads();
    for (int e = threadIdx.x; e < tpad * 3; e += kChBlock)
      sk[e] = e < tn * 3 ? ref[(long long)t0 * 3 + e] : INFINITY;
    __syncthreads();
    for (int j0 = 0; active && j0 < tpad; j0 += kChChunk) {
      float r[kChChunk * 3];
#pragma unroll
      for (int v = 0; v < kChChunk * 3 / 4; ++v) {
        const float4 x = sk4[j0 * 3 / 4 + v];
        r[4 * v + 0] = x.x; r[4 * v + 1] = x.y; r[4 * v + 2] = x.z; r[4 * v + 3] = x.w;
      }
      float d[kChChunk];
#pragma unroll
      for (int u = 0; u < kChChunk; ++u)
        d[u] = dist3(r[3 * u + 0], r[3 * u + 1], r[3 * u + 2], qx, qy, qz);
      // fminf drops NaNs and a NaN distance passes no test below; the padding's distance is
      // +inf (or NaN), never < best
      float dmin = d[0];
#pragma unroll
      for (int u = 1; u < kChChunk; ++u) dmin = fminf(dmin, d[u]);
      if (!(dmin < best)) continue;
#pragma unroll
      for (int u = 0; u < kChChunk; ++u) {  // ascending index, strict <
        if (d[u] < best) {
          best = d[u];
          ibest = t0 + j0 + u;
        }
      }
    }
  }
  if (!active) return;
  const long long o = (long long)bi * nq + row;
  (ba ? dist_ba : dist_ab)[o] = best;
  (ba ? idx_ba : idx_ab)[o] = ibest;
}

__global__ __launch_bounds__(kChBlock) void chamfer_bwd_kernel(
    int b, int n, int m, const float* __restrict__ a, const float* __restrict__ bp,
    const int* __restrict__ idx_ab, const float* __restrict__ g_ab,
    const int* __restrict__ offsets_ba, const int* __restrict__ perm_ba,
    const float* __restrict__ g_ba, float* __restrict__ da) {
  const int total = b * n;
  const int row = blockIdx.x * kChBlock + threadIdx.x;  // bi * n + i, the CSR key
  if (row >= total) return;
  const int bi = row / n;
  const float ax = a[(long long)row * 3 + 0];
  const float ay = a[(long long)row * 3 + 1];
  const float az = a[(long long)row * 3 + 2];
  // indices are read-only inputs: clamped, so no value of them reads outside bp / g_ba
  const int j = min(max(idx_ab[row], 0), m - 1);
  const float* br = bp + ((long long)bi * m + j) * 3;
  const float w = 2.0f * g_ab[row];
  float gx = __fmul_rn(w, ax - br[0]);
  float gy = __fmul_rn(w, ay - br[1]);
  float gz = __fmul_rn(w, az - br[2]);
  if (offsets_ba) {
    const int p1 = offsets_ba[row + 1];
    for (int p = offsets_ba[row]; p < p1; ++p) {
      const int pos = min(max(perm_ba[p], 0), b * m - 1);  // flat row of bp / g_ba
      const float* bq = bp + (long long)pos * 3;
      const float w2 = 2.0f * g_ba[pos];
      gx = __builtin_fmaf(w2, ax - bq[0], gx);
      gy = __builtin_fmaf(w2, ay - bq[1], gy);
      gz = __builtin_fmaf(w2, az - bq[2], gz);
    }
  }
  da[(long long)row * 3 + 0] = gx;
  da[(long long)row * 3 + 1] = gy;
  da[(long long)row * 3 + 2] = gz;
}

// b * max(n, m) is an int row index (and the CSR's key / position space)
bool chamfer_sizes_ok(int b, int n, int m) {
  return b >= 0 && b <= 65535 && n >= 1 && m >= 1 &&
         (long long)b * (n > m ? n : m) <= 0x7fffffffLL;
}

}  // namespace

KDPC_API int kdpc_chamfer_fwd(int b, int n, int m, const float* a, const float* bp,
                              float* dist_ab, int* idx_ab, float* dist_ba, int* idx_ba,
                              void* stream) {
  KDPC_CHECK_ARG(chamfer_sizes_ok(b, n, m));
  if (b == 0) return (int)hipSuccess;
  KDPC_CHECK_ARG(a && bp && dist_ab && idx_ab && dist_ba && idx_ba);
  const unsigned gx = (unsigned)divup(n > m ? n : m, kChBlock);
  hipLaunchKernelGGL(chamfer_fwd_kernel, dim3(gx, b, 2), dim3(kChBlock), 0, (hipStream_t)stream,
                     n, m, a, bp, dist_ab, idx_ab, dist_ba, idx_ba);
  KDPC_RETURN_LAUNCH();
}

KDPC_API int kdpc_chamfer_bwd(int b, int n, int m, const float* a, const float* bp,
                              const int* idx_ab, const float* g_ab, const int* offsets_ba,
                              const int* perm_ba, const float* g_ba, float* da, void* stream) {
  KDPC_CHECK_ARG(chamfer_sizes_ok(b, n, m));
  // the b -> a direction is given whole or not at all
  const int nba = (g_ba != nullptr) + (offsets_ba != nullptr) + (perm_ba != nullptr);
  KDPC_CHECK_ARG(nba == 0 || nba == 3);
  if (b == 0) return (int)hipSuccess;
  KDPC_CHECK_ARG(a && bp && idx_ab && g_ab && da);
  const unsigned gx = (unsigned)divupll((long long)b * n, kChBlock);
  hipLaunchKernelGGL(chamfer_bwd_kernel, dim3(gx), dim3(kChBlock), 0, (hipStream_t)stream, b, n,
                     m, a, bp, idx_ab, g_ab, offsets_ba, perm_ba, g_ba, da);
  KDPC_RETURN_LAUNCH();
}
