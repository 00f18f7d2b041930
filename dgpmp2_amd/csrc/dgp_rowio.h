// dgp_rowio.h -- how a side kernel moves one row of D elements between memory and registers: as vectors where the caller found every pointer of the call aligned
// to the vector (`vec`), element by element otherwise: the same bits either way.  One rule for the width, vec_bytes: 16-byte vectors where the row's byte length is
// a multiple of 16, 8-byte ones otherwise (the 24-byte fp32 row of d = 6, whose every second row sits off the 16-byte boundary; the 8-byte fp32 point of
// sdf_lookup.hip).  HIP only, nothing of the solver, no arithmetic.  gn_lane.h has its own RowVec / ld_row for the step kernels.
// The wording is held to the kernels' assembly: HIP's own vector types, every vector of a row loaded before the first is unpacked, a stored vector built by its
// constructor.  Under it heading_lift.hip and prior_samples.hip compile to the code they had with their own copies; step_loss.hip and sdf_lookup.hip do not (they
// keep their ext_vector_type wording of the same accesses and share the rule).
#pragma once
#include <hip/hip_runtime.h>

namespace dgp_rowio {

template <typename IO, int D>
constexpr int vec_bytes() { return (D * sizeof(IO)) % 16 == 0 ? 16 : 8; }

template <typename IO, int BYTES> struct Vec;
template <> struct Vec<float, 8> { typedef float2 type; };
template <> struct Vec<float, 16> { typedef float4 type; };
template <> struct Vec<double, 16> { typedef double2 type; };

template <typename IO, int D>
__device__ __forceinline__ void load_row(const IO* src, IO (&v)[D], bool vec) {
  if (vec) {
    typedef typename Vec<IO, vec_bytes<IO, D>()>::type vec_t;
    constexpr int VE = (int)(sizeof(vec_t) / sizeof(IO));
    vec_t q[D / VE];
#pragma unroll
    for (int j = 0; j < D / VE; ++j) q[j] = *reinterpret_cast<const vec_t*>(src + j * VE);
#pragma unroll
    for (int j = 0; j < D / VE; ++j) {
      v[j * VE] = q[j].x; v[j * VE + 1] = q[j].y;
      if constexpr (VE == 4) { v[j * VE + 2] = q[j].z; v[j * VE + 3] = q[j].w; }
    }
  } else {
#pragma unroll
    for (int c = 0; c < D; ++c) v[c] = src[c];
  }
}

template <typename IO, int D>
__device__ __forceinline__ void store_row(IO* dst, const IO (&v)[D], bool vec) {
  if (vec) {
    typedef typename Vec<IO, vec_bytes<IO, D>()>::type vec_t;
    constexpr int VE = (int)(sizeof(vec_t) / sizeof(IO));
#pragma unroll
    for (int c = 0; c < D; c += VE) {
      if constexpr (VE == 4) *reinterpret_cast<vec_t*>(dst + c) = vec_t(v[c], v[c + 1], v[c + 2], v[c + 3]);
      else *reinterpret_cast<vec_t*>(dst + c) = vec_t(v[c], v[c + 1]);
    }
  } else {
#pragma unroll
    for (int c = 0; c < D; ++c) dst[c] = v[c];
  }
}

}  // namespace dgp_rowio
