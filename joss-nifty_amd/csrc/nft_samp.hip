// Sampling responses: MaskOperator (src/operators/mask_operator.py) and
// LinearInterpolator (src/operators/linear_interpolation.py; the reference
// applies a scipy COO matrix with 2^ndim entries per point).
//
// Every data point reads 1 (mask) or 2^ndim (multilinear interpolation) grid
// values.  No matrix is stored: the plan holds per point its cell index per
// axis and, for the interpolation, its ndim fp64 fractions; the weights
//   w_c = prod over axes of (bit_c(axis) ? e : 1 - e)      (axis order, fp64)
// are recomputed where they are used, bitwise the reference's (_build_mat).
// The plan lists the points sorted by pixel tile (point[s] = the datum at
// position s): the lanes of a wave then gather from a few neighbouring grid
// lines instead of one random line each, in both directions.
//
//  forward  y = rs * R (cs * x):  one thread per point; the 2^ndim corner
//    values are gathered and summed in corner order (the COO order).
//    Optional per-block partials of t_p * y_p (the data-space curvature of
//    the sampling-metric middle, as nft_los_forward_quad_batched).
//  adjoint  out = rs * R^T (cs * y):  sort-by-destination -- the entries are
//    regrouped by grid pixel on the host (pix_ptr, a CSR over ALL pixels;
//    ent = position * ncorner + corner, ascending (corner, datum) within a
//    pixel: the COO order); one thread per pixel sums its run serially and
//    stores the pixel, untouched pixels store 0.  One pass, every pixel
//    written, no atomics, no cap on the entries of a pixel.
//
// All sums run in a fixed order and no product is contracted into an FMA:
// results are bitwise reproducible and, per vector, independent of nvec.
#include <algorithm>

#include "nft_api_internal.hpp"

namespace nft {

constexpr int SAMP_KMAX = 8;  // vectors per batched launch

// the corner's bit of axis d: np.mgrid ravel order, the first axis slowest
template <int ND>
__device__ __forceinline__ int corner_bit(int c, int d) {
  return (c >> (ND - 1 - d)) & 1;
}

// cell indices and fractions of the point at position pt of the plan (ND >= 1)
template <int ND>
struct SampPoint {
  int i0[ND], i1[ND];
  double e[ND];
  __device__ __forceinline__ void load(const nft_samp_plan& p, long long pt) {
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      const int i = p.idx[d * p.npoints + pt];
      i0[d] = i;
      i1[d] = (i + 1 >= (int)p.shape[d]) ? 0 : i + 1;  // periodic
      e[d] = p.frac[d * p.npoints + pt];
    }
  }
  __device__ __forceinline__ long long pixel(const nft_samp_plan& p, int c) const {
    long long j = 0;
#pragma unroll
    for (int d = 0; d < ND; ++d) j = j * p.shape[d] + (corner_bit<ND>(c, d) ? i1[d] : i0[d]);
    return j;
  }
  __device__ __forceinline__ double weight(int c) const {
#pragma clang fp contract(off)
    double w = corner_bit<ND>(c, 0) ? e[0] : 1.0 - e[0];
#pragma unroll
    for (int d = 1; d < ND; ++d) w = w * (corner_bit<ND>(c, d) ? e[d] : 1.0 - e[d]);
    return w;
  }
};

// ND = 0: the mask (one corner, weight 1, idx = the flat pixel).  kv <= K
// vectors are valid.  qpart (optional): qpart[v * qstride + block] = the sum
// over the block's 256 points of t_p * y_p (t the sum before scale *
// rowscale, y the stored output): four wave shuffle trees, then the wave
// totals in order, per vector -- the same for every K.
template <typename T, int ND, int K>
__global__ __launch_bounds__(256) void samp_fwd(nft_samp_plan p, const T* __restrict__ x, const T* __restrict__ cs,
                                                const T* __restrict__ rs, T* __restrict__ y, double scale,
                                                long long xs, long long ys, long long css, int kv,
                                                double* __restrict__ qpart, long long qstride) {
#pragma clang fp contract(off)
  constexpr int NC = 1 << ND;
  __shared__ double qs[4][K];
  const int t = threadIdx.x;
  // sp: the point's position in the plan's (pixel-sorted) order, pt: its datum
  const long long sp = (long long)blockIdx.x * 256 + t;
  const bool valid = sp < p.npoints;
  const long long pt = (valid && p.point) ? p.point[sp] : sp;
  double acc[K];
#pragma unroll
  for (int v = 0; v < K; ++v) acc[v] = 0.0;
  if (valid) {
    if constexpr (ND == 0) {
      const long long j = p.idx[sp];
#pragma unroll
      for (int v = 0; v < K; ++v) {
        if (v < kv) {
          double u = (double)x[v * xs + j];
          if (cs) u *= (double)cs[v * css + j];
          acc[v] = u;
        }
      }
    } else {
      SampPoint<ND> q;
      q.load(p, sp);
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const long long j = q.pixel(p, c);
        const double w = q.weight(c);
#pragma unroll
        for (int v = 0; v < K; ++v) {
          if (v < kv) {
            double u = (double)x[v * xs + j];
            if (cs) u *= (double)cs[v * css + j];
            acc[v] = acc[v] + w * u;
          }
        }
      }
    }
  }
  double q[K];
#pragma unroll
  for (int v = 0; v < K; ++v) {
    q[v] = 0.0;
    if (valid && v < kv) {
      double yy = acc[v] * scale;
      if (rs) yy *= (double)rs[pt];
      y[v * ys + pt] = (T)yy;
      q[v] = acc[v] * (double)(T)yy;
    }
  }
  if (qpart) {  // uniform over the block
#pragma unroll
    for (int v = 0; v < K; ++v) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) q[v] += __shfl_down(q[v], off, 64);
      if ((t & 63) == 0) qs[t >> 6][v] = q[v];
    }
    __syncthreads();
    if (t < K && t < kv) qpart[t * qstride + blockIdx.x] = ((qs[0][t] + qs[1][t]) + qs[2][t]) + qs[3][t];
  }
}

// one thread per grid pixel; a plan without points (pix_ptr NULL) stores zeros
template <typename T, int ND, int K>
__global__ __launch_bounds__(256) void samp_adj(nft_samp_plan p, const T* __restrict__ yv, const T* __restrict__ cs,
                                                const T* __restrict__ rs, T* __restrict__ out, double scale,
                                                long long ys, long long os, long long rss, int kv) {
#pragma clang fp contract(off)
  constexpr int NC = 1 << ND;
  const long long px = (long long)blockIdx.x * 256 + threadIdx.x;
  if (px >= p.npix) return;
  int a = 0, b = 0;
  if (p.npoints > 0) {
    a = p.pix_ptr[px];
    b = p.pix_ptr[px + 1];
  }
  double acc[K];
#pragma unroll
  for (int v = 0; v < K; ++v) acc[v] = 0.0;
  for (int k = a; k < b; ++k) {
    const int en = p.ent[k];
    const long long sp = en >> ND;  // position in the plan's order
    const long long pt = p.point ? p.point[sp] : sp;
    double w = 1.0;
    if constexpr (ND > 0) {
      const int c = en & (NC - 1);
      w = corner_bit<ND>(c, 0) ? p.frac[sp] : 1.0 - p.frac[sp];
#pragma unroll
      for (int d = 1; d < ND; ++d) {
        const double e = p.frac[d * p.npoints + sp];
        w = w * (corner_bit<ND>(c, d) ? e : 1.0 - e);
      }
    }
    const double cc = cs ? (double)cs[pt] : 1.0;
#pragma unroll
    for (int v = 0; v < K; ++v) {
      if (v < kv) {
        double yy = (double)yv[v * ys + pt];
        if (cs) yy *= cc;
        if constexpr (ND == 0)
          acc[v] = yy;  // at most one entry per pixel
        else
          acc[v] = acc[v] + w * yy;
      }
    }
  }
#pragma unroll
  for (int v = 0; v < K; ++v) {
    if (v < kv) {
      double o = acc[v] * scale;
      if (rs) o *= (double)rs[v * rss + px];
      out[v * os + px] = (T)o;
    }
  }
}

// vector groups as the LOS kernels: 8 / 4 / 2 / 1, a remainder of 5-7 (3)
// vectors in one launch of the 8 (4) instance with the missing ones masked
static int samp_kgroup(int k) { return k >= 5 ? 8 : (k >= 3 ? 4 : (k == 2 ? 2 : 1)); }

template <typename T, int ND>
static int samp_forward_nd(const nft_samp_plan* p, const T* x, const T* cs, const T* rs, T* y, double scale, int K,
                           long long xs, long long ys, long long css, double* qpart, long long qs, hipStream_t s) {
  const dim3 grid((unsigned)((p->npoints + 255) / 256));
  for (int v = 0; v < K;) {
    const int g = samp_kgroup(K - v), kv = std::min(g, K - v);
    const T* xv = x + v * xs;
    const T* cv = cs ? cs + v * css : nullptr;
    T* yv = y + v * ys;
    double* qv = qpart ? qpart + v * qs : nullptr;
#define NFT_SAMP_FWD(KK)                                                                                         \
  hipLaunchKernelGGL((samp_fwd<T, ND, KK>), grid, dim3(256), 0, s, *p, xv, cv, rs, yv, scale, xs, ys, css, kv, \
                     qv, qs)
    switch (g) {
      case 8: NFT_SAMP_FWD(8); break;
      case 4: NFT_SAMP_FWD(4); break;
      case 2: NFT_SAMP_FWD(2); break;
      default: NFT_SAMP_FWD(1); break;
    }
#undef NFT_SAMP_FWD
    v += kv;
  }
  NFT_HIP_CHECK(hipGetLastError());
  return NFT_OK;
}

template <typename T, int ND>
static int samp_adjoint_nd(const nft_samp_plan* p, const T* y, const T* cs, const T* rs, T* out, double scale, int K,
                           long long ys, long long os, long long rss, hipStream_t s) {
  const dim3 grid((unsigned)((p->npix + 255) / 256));
  for (int v = 0; v < K;) {
    const int g = samp_kgroup(K - v), kv = std::min(g, K - v);
    const T* yv = y + v * ys;
    const T* rv = rs ? rs + v * rss : nullptr;
    T* ov = out + v * os;
#define NFT_SAMP_ADJ(KK) \
  hipLaunchKernelGGL((samp_adj<T, ND, KK>), grid, dim3(256), 0, s, *p, yv, cs, rv, ov, scale, ys, os, rss, kv)
    switch (g) {
      case 8: NFT_SAMP_ADJ(8); break;
      case 4: NFT_SAMP_ADJ(4); break;
      case 2: NFT_SAMP_ADJ(2); break;
      default: NFT_SAMP_ADJ(1); break;
    }
#undef NFT_SAMP_ADJ
    v += kv;
  }
  NFT_HIP_CHECK(hipGetLastError());
  return NFT_OK;
}

template <typename T>
static int samp_forward_t(const nft_samp_plan* p, const void* x, const void* cs, const void* rs, void* y,
                          double scale, int K, long long xs, long long ys, long long css, double* qpart,
                          long long qs, hipStream_t s) {
  prof_mark(s, "samp_fwd");
  const int nd = p->ncorner == 1 ? 0 : p->ndim;
#define NFT_SAMP_ND(N) \
  return samp_forward_nd<T, N>(p, (const T*)x, (const T*)cs, (const T*)rs, (T*)y, scale, K, xs, ys, css, qpart, qs, s)
  switch (nd) {
    case 0: NFT_SAMP_ND(0);
    case 1: NFT_SAMP_ND(1);
    case 2: NFT_SAMP_ND(2);
    default: NFT_SAMP_ND(3);
  }
#undef NFT_SAMP_ND
}

template <typename T>
static int samp_adjoint_t(const nft_samp_plan* p, const void* y, const void* cs, const void* rs, void* out,
                          double scale, int K, long long ys, long long os, long long rss, hipStream_t s) {
  prof_mark(s, "samp_adj");
  const int nd = p->ncorner == 1 ? 0 : p->ndim;
#define NFT_SAMP_ND(N) \
  return samp_adjoint_nd<T, N>(p, (const T*)y, (const T*)cs, (const T*)rs, (T*)out, scale, K, ys, os, rss, s)
  switch (nd) {
    case 0: NFT_SAMP_ND(0);
    case 1: NFT_SAMP_ND(1);
    case 2: NFT_SAMP_ND(2);
    default: NFT_SAMP_ND(3);
  }
#undef NFT_SAMP_ND
}

// geometry and arrays of a plan; `what` names the entry point in the message
static int samp_check_plan(const nft_samp_plan* p, const char* what) {
  if (!p || p->ndim < 1 || p->ndim > 3 || p->npoints < 0 || p->npix < 0) {
    set_last_error("%s: invalid plan (1 <= ndim <= 3, npoints >= 0, npix >= 0)", what);
    return NFT_ERR_ARG;
  }
  long long n = 1;
  for (int d = 0; d < p->ndim; ++d) {
    if (p->shape[d] < 0 || p->shape[d] > 0x7fffffffLL) {
      set_last_error("%s: invalid plan (axis lengths must fit int32)", what);
      return NFT_ERR_ARG;
    }
    n *= p->shape[d];
  }
  const bool mask = p->ncorner == 1;
  if (n != p->npix || (!mask && p->ncorner != (1 << p->ndim)) || (mask && p->ndim != 1)) {
    set_last_error("%s: invalid plan (npix = prod(shape); ncorner = 2^ndim, or 1 on a flat grid)", what);
    return NFT_ERR_ARG;
  }
  if (p->npoints * p->ncorner > 0x7fffffffLL) {
    set_last_error("%s: more than 2^31 - 1 entries", what);
    return NFT_ERR_ARG;
  }
  if (p->npoints > 0 && (!p->idx || !p->pix_ptr || !p->ent || (!mask && !p->frac))) {
    set_last_error("%s: plan arrays missing (idx, pix_ptr, ent; frac for an interpolation)", what);
    return NFT_ERR_ARG;
  }
  return NFT_OK;
}

}  // namespace nft

using namespace nft;

extern "C" {

int nft_samp_quad_blocks(const nft_samp_plan* p) {
  return (p && p->npoints > 0) ? (int)((p->npoints + 255) / 256) : 0;
}

int nft_samp_forward_batched(const nft_samp_plan* p, const void* x, const void* colscale, int64_t colscale_stride,
                             const void* rowscale, void* y, int dtype, double scale, int nvec, int64_t x_stride,
                             int64_t y_stride, double* qpart, int64_t qstride, hipStream_t stream) {
  int st = samp_check_plan(p, "nft_samp_forward");
  if (st != NFT_OK) return st;
  if (nvec < 1 || nvec > SAMP_KMAX || (nvec > 1 && (x_stride < 1 || y_stride < 1)) ||
      (colscale && colscale_stride < 0) || (qpart && qstride < nft_samp_quad_blocks(p)) ||
      (qpart && nvec > 1 && qstride < 1)) {
    set_last_error("nft_samp_forward: 1 <= nvec <= %d, x / y strides >= 1 for nvec > 1, colscale_stride >= 0, "
                   "qstride >= nft_samp_quad_blocks", SAMP_KMAX);
    return NFT_ERR_ARG;
  }
  if (dtype != 0 && dtype != 1) {
    set_last_error("nft_samp_forward: bad dtype %d", dtype);
    return NFT_ERR_ARG;
  }
  if (p->npoints == 0) return NFT_OK;  // no data: nothing to write
  if (!x || !y) {
    set_last_error("nft_samp_forward: x and y required");
    return NFT_ERR_ARG;
  }
  if (dtype == 0)
    return samp_forward_t<double>(p, x, colscale, rowscale, y, scale, nvec, x_stride, y_stride, colscale_stride,
                                  qpart, qstride, stream);
  return samp_forward_t<float>(p, x, colscale, rowscale, y, scale, nvec, x_stride, y_stride, colscale_stride, qpart,
                               qstride, stream);
}

int nft_samp_adjoint_batched(const nft_samp_plan* p, const void* y, const void* colscale, const void* rowscale,
                             int64_t rowscale_stride, void* out, int dtype, double scale, int nvec, int64_t y_stride,
                             int64_t out_stride, hipStream_t stream) {
  int st = samp_check_plan(p, "nft_samp_adjoint");
  if (st != NFT_OK) return st;
  if (nvec < 1 || nvec > SAMP_KMAX || (nvec > 1 && (y_stride < 1 || out_stride < 1)) ||
      (rowscale && rowscale_stride < 0)) {
    set_last_error("nft_samp_adjoint: 1 <= nvec <= %d, y / out strides >= 1 for nvec > 1, rowscale_stride >= 0",
                   SAMP_KMAX);
    return NFT_ERR_ARG;
  }
  if (dtype != 0 && dtype != 1) {
    set_last_error("nft_samp_adjoint: bad dtype %d", dtype);
    return NFT_ERR_ARG;
  }
  if (p->npix == 0) return NFT_OK;  // no pixels: nothing to write
  if (!out || (p->npoints > 0 && !y)) {
    set_last_error("nft_samp_adjoint: y and out required");
    return NFT_ERR_ARG;
  }
  if (dtype == 0)
    return samp_adjoint_t<double>(p, y, colscale, rowscale, out, scale, nvec, y_stride, out_stride, rowscale_stride,
                                  stream);
  return samp_adjoint_t<float>(p, y, colscale, rowscale, out, scale, nvec, y_stride, out_stride, rowscale_stride,
                               stream);
}

}  // extern "C"
