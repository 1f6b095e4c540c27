// Device arithmetic of the 3-NN inverse-distance blend (UpsampleFlow / PointWarping,
// reference pointconv_util.py:2130-2139 and 2165-2170), shared by idw_blend.hip (dense, given
// indices) and flow_propagate.hip (ragged, fused with the 3-NN search) so the two cannot
// drift:
//
//   g_k = ref[idx_k] - q,  d_k = max(||g_k||, 1e-10),  r_k = 1 / d_k,
//   w_k = r_k / (r_0 + r_1 + r_2),  blend = sum_k w_k vals[idx_k]
//
// Arithmetic follows the torch expression's order (products rounded, then summed in k order;
// no contraction: the library is built with -ffp-contract=off).
#pragma once
#include "kdpc_common.h"

namespace kdpc {

constexpr float kIdwMinDist = 1e-10f;  // .clamp(min=1e-10) of the reference

struct Geo3 {
  float g[3][3];  // g_k = ref[idx_k] - q
  float len[3];   // ||g_k||
  float r[3];     // 1 / max(||g_k||, 1e-10)
  float w[3];     // r_k / sum r
  float sum;      // r_0 + r_1 + r_2
  int nb[3];      // global reference rows b*S + idx_k
};

// the geometry of one query (qx, qy, qz) against the reference rows o.nb[0..2] (set by the
// caller, each a valid row of ref)
__device__ __forceinline__ void idw_geometry_rows(const float* __restrict__ ref, float qx,
                                                  float qy, float qz, Geo3& o) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int nb = o.nb[k];
    const float gx = ref[(long long)nb * 3 + 0] - qx;
    const float gy = ref[(long long)nb * 3 + 1] - qy;
    const float gz = ref[(long long)nb * 3 + 2] - qz;
    o.g[k][0] = gx;
    o.g[k][1] = gy;
    o.g[k][2] = gz;
    const float len = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(gx, gx), __fmul_rn(gy, gy)),
                                           __fmul_rn(gz, gz)));
    o.len[k] = len;
    o.r[k] = __fdiv_rn(1.0f, fmaxf(len, kIdwMinDist));
  }
  o.sum = __fadd_rn(__fadd_rn(o.r[0], o.r[1]), o.r[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) o.w[k] = __fdiv_rn(o.r[k], o.sum);
}

// dense layout: query `row` of qry (B,N,3), its neighbours idx[row*3 + k] in [0,S) of cloud bi
__device__ __forceinline__ void idw_geometry(const float* __restrict__ ref,
                                             const float* __restrict__ qry,
                                             const int* __restrict__ idx, long long row, int s,
                                             int bi, Geo3& o) {
  const float qx = qry[row * 3 + 0], qy = qry[row * 3 + 1], qz = qry[row * 3 + 2];
#pragma unroll
  for (int k = 0; k < 3; ++k) o.nb[k] = bi * s + idx[row * 3 + k];
  idw_geometry_rows(ref, qx, qy, qz, o);
}

// (w_0 a_0 + w_1 a_1) + w_2 a_2, every product and sum rounded
__device__ __forceinline__ float idw_blend3(const Geo3& o, float a0, float a1, float a2) {
  return __fadd_rn(__fadd_rn(__fmul_rn(o.w[0], a0), __fmul_rn(o.w[1], a1)),
                   __fmul_rn(o.w[2], a2));
}

}  // namespace kdpc
