// Full-scan flow propagation: what the model predicted for the N anchor points it was fed,
// carried to every point of a ragged batch of scans by the model's own UpsampleFlow rule.
// One kernel = kdpc_three_nn's search (pointnet2_ops.hip three_nn_kernel) fused with
// kdpc_idw_blend_fwd's blend (idw_math.h, warp = 0):
//
//   (i_0, i_1, i_2) = the 3 anchors of the query's cloud with the smallest dist3(anchor, q),
//                     strict <, so the lower anchor index wins ties
//   out[row, :]     = sum_k w_k vals[i_k, :],  w_k = (1/d_k) / sum_j (1/d_j),
//                     d_k = max(||anchor[i_k] - q||, 1e-10)
//
// Ragged: the queries of all clouds are packed into (m_total, 3) and cloud i owns the rows
// offsets[i] .. offsets[i+1] (device int64); grid = (ceil(max_len / 256), B), one thread per
// query row, rows past the cloud's end exit.  The offsets cannot be checked by the host: the
// kernel clamps every cloud's range to [0, m_total), so no value of offsets makes it touch a
// row outside qry / out / idx_out.
//
// Scan: the cloud's anchors staged through LDS in 1024-anchor tiles (12 KiB) and read back as
// broadcasts (every lane the same address: no bank conflicts), as three_nn_kernel does, but
// 8 anchors at a time: their 6 16-byte reads are in flight together and the 8 distances are
// formed before anything is tested, then one test (min of the 8 against the third best)
// skips the update in the common case.  three_nn_kernel reads, waits and branches per anchor,
// so with the one or two waves per SIMD a 90k-point scan gives, it pays the LDS latency 8192
// times.  The update itself is three_nn_kernel's, in ascending anchor order, so the
// selection is identical; the three running bests live in registers.  Nothing goes through HBM
// between the search and the blend (the unfused pair writes and re-reads idx, dist2 and w:
// 36 bytes per query for a 12-byte result).  Writes out (and idx_out when given) only: no
// workspace, no allocation, no atomics.
#include "idw_math.h"
#include "kdpc_common.h"

using namespace kdpc;

namespace {

constexpr int kFpTile = 1024;  // anchors per LDS tile (three_nn_kernel's kNNTile)
constexpr int kFpBlock = 256;
constexpr int kFpChunk = 8;  // anchors whose distances are formed together (96 bytes of LDS)
static_assert(kFpTile % kFpChunk == 0 && (kFpChunk * 3) % 4 == 0, "chunks are whole float4s");

__global__ __launch_bounds__(kFpBlock) void flow_propagate_kernel(
    int n, int c, long long m_total, const float* __restrict__ anchors,
    const float* __restrict__ vals, const float* __restrict__ qry,
    const long long* __restrict__ offsets, float* __restrict__ out, int* __restrict__ idx_out) {
  __shared__ float4 sk4[kFpTile * 3 / 4];
  float* sk = reinterpret_cast<float*>(sk4);
  const int bi = blockIdx.y;
  // this cloud's rows, clamped to [0, m_total) whatever offsets holds
  long long r0 = offsets[bi], r1 = offsets[bi + 1];
  r0 = r0 < 0 ? 0 : (r0 > m_total ? m_total : r0);
  r1 = r1 < r0 ? r0 : (r1 > m_total ? m_total : r1);
  const long long first = r0 + (long long)blockIdx.x * kFpBlock;
  if (first >= r1) return;  // block-uniform: before any barrier
  const long long row = first + threadIdx.x;
  const bool active = row < r1;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (active) {
    qx = qry[row * 3 + 0];
    qy = qry[row * 3 + 1];
    qz = qry[row * 3 + 2];
  }
  const float* ab = anchors + (long long)bi * n * 3;
  float b1 = INFINITY, b2 = INFINITY, b3 = INFINITY;
  int i1 = 0, i2 = 0, i3 = 0;
  for (int t0 = 0; t0 < n; t0 += kFpTile) {
    const int tn = min(kFpTile, n - t0);
    const int tpad = divup(tn, kFpChunk) * kFpChunk;  // <= kFpTile
    __syncthreads();
    for (int e = threadIdx.x; e < tpad * 3; e += kFpBlock)
      sk[e] = e < tn * 3 ? ab[(long long)t0 * 3 + e] : INFINITY;
    __syncthreads();
    for (int j0 = 0; active && j0 < tpad; j0 += kFpChunk) {
      // kFpChunk anchors = 6 x 16 bytes, read as broadcasts and all in flight together; their
      // distances are formed before any test, so the LDS latency is paid once per chunk
      float a[kFpChunk * 3];
#pragma unroll
      for (int v = 0; v < kFpChunk * 3 / 4; ++v) {
        const float4 x = sk4[j0 * 3 / 4 + v];
        a[4 * v + 0] = x.x; a[4 * v + 1] = x.y; a[4 * v + 2] = x.z; a[4 * v + 3] = x.w;
      }
      float d[kFpChunk];
#pragma unroll
      for (int u = 0; u < kFpChunk; ++u)
        d[u] = dist3(a[3 * u + 0], a[3 * u + 1], a[3 * u + 2], qx, qy, qz);
      // b1 <= b2 <= b3 always, so only an anchor with d < b3 changes anything: one test per
      // chunk in the common case.  fminf drops NaNs and a NaN distance passes no test below;
      // the padding's distance is +inf (or NaN), never < b3
      float dmin = d[0];
#pragma unroll
      for (int u = 1; u < kFpChunk; ++u) dmin = fminf(dmin, d[u]);
      if (!(dmin < b3)) continue;
      // three_nn_kernel's update, in ascending anchor order
#pragma unroll
      for (int u = 0; u < kFpChunk; ++u) {
        const float du = d[u];
        const int k = t0 + j0 + u;
        if (du < b1) {
          b3 = b2; i3 = i2; b2 = b1; i2 = i1; b1 = du; i1 = k;
        } else if (du < b2) {
          b3 = b2; i3 = i2; b2 = du; i2 = k;
        } else if (du < b3) {
          b3 = du; i3 = k;
        }
      }
    }
  }
  if (!active) return;
  if (idx_out) {
    idx_out[row * 3 + 0] = i1;
    idx_out[row * 3 + 1] = i2;
    idx_out[row * 3 + 2] = i3;
  }
  Geo3 o;
  o.nb[0] = bi * n + i1;  // i_k in [0, n): rows of this cloud's anchors / vals
  o.nb[1] = bi * n + i2;
  o.nb[2] = bi * n + i3;
  idw_geometry_rows(anchors, qx, qy, qz, o);
  const float* v0 = vals + (long long)o.nb[0] * c;
  const float* v1 = vals + (long long)o.nb[1] * c;
  const float* v2 = vals + (long long)o.nb[2] * c;
  float* orow = out + row * c;
  if ((c & 3) == 0) {  // 16-byte value rows
    for (int ch = 0; ch < c; ch += 4) {
      const float4 x0 = *reinterpret_cast<const float4*>(v0 + ch);
      const float4 x1 = *reinterpret_cast<const float4*>(v1 + ch);
      const float4 x2 = *reinterpret_cast<const float4*>(v2 + ch);
      *reinterpret_cast<float4*>(orow + ch) =
          make_float4(idw_blend3(o, x0.x, x1.x, x2.x), idw_blend3(o, x0.y, x1.y, x2.y),
                      idw_blend3(o, x0.z, x1.z, x2.z), idw_blend3(o, x0.w, x1.w, x2.w));
    }
    return;
  }
  for (int ch = 0; ch < c; ++ch) orow[ch] = idw_blend3(o, v0[ch], v1[ch], v2[ch]);
}

}  // namespace

KDPC_API int kdpc_flow_propagate(int b, int n, int c, long long m_total, int max_len,
                                 const float* anchors, const float* vals, const float* qry,
                                 const long long* offsets, float* out, int* idx_out,
                                 void* stream) {
  KDPC_CHECK_ARG(b >= 0 && b <= 65535 && m_total >= 0 && max_len >= 0 && n >= 3 && c >= 1);
  // bi * n + i_k is an int row index (as in kdpc_idw_blend_fwd)
  KDPC_CHECK_ARG((long long)b * n <= 0x7fffffffLL);
  if (b == 0 || m_total == 0 || max_len == 0) return (int)hipSuccess;
  KDPC_CHECK_ARG(anchors && vals && qry && offsets && out);
  const unsigned gx = (unsigned)divupll(max_len, kFpBlock);
  hipLaunchKernelGGL(flow_propagate_kernel, dim3(gx, b), dim3(kFpBlock), 0, (hipStream_t)stream,
                     n, c, m_total, anchors, vals, qry, offsets, out, idx_out);
  KDPC_RETURN_LAUNCH();
}
