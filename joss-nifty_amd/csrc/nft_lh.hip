// Pointwise likelihood terms on batches of model outputs.
//
// Replaces, for BernoulliEnergy, StudentTEnergy and InverseGammaEnergy
// (src/operators/energy_operators.py:628-761):
//   the value / gradient passes of LikelihoodEnergyOperator.apply on the k
//   sample positions of a sampled KL (src/minimization/kl_energies.py:295-356)
//   the Fisher weight of get_metric_at (the squared Jacobian of
//   get_transformation)
//   the value and Jacobian of BernoulliEnergy.get_transformation
//   (-2 arctan sqrt((1 - f) / f), energy_operators.py:757-761)
//
// Every transcendental and every sum is fp64, also for fp32 storage.  The
// energy is a two-level reduction like nft_dot_batched: per-workgroup fp64
// partials (wave64 shuffles + LDS) in the caller's workspace, then one
// workgroup per row folds them in index order -- bitwise reproducible, no
// atomics.  A thread owns whole 16-byte chunks of a row and the chunk -> thread
// map depends on n alone, so a row's sum has one order whatever the batch and
// whatever the alignment (unaligned rows take scalar loads of the same chunks).
#include "nft_api_internal.hpp"
#include "../../include/nifty_amd.h"

namespace nft {
namespace {

constexpr int LH_NT = 256;

__device__ __forceinline__ double lh_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// sum over the workgroup, valid in thread 0 (waves in index order)
__device__ __forceinline__ double lh_block_sum(double v, double* sh) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  v = lh_wave_sum(v);
  if (lane == 0) sh[wid] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < LH_NT / 64; ++w) s += sh[w];
  return s;
}

template <typename T, int V> struct alignas(16) Pack { T v[V]; };

// V consecutive values at p[i0..]; VEC: one or two 16-byte loads (all V in range)
template <typename T, int V, bool VEC>
__device__ __forceinline__ void load_chunk(const T* __restrict__ p, long long i0, long long n, T (&o)[V]) {
  constexpr int W = 16 / (int)sizeof(T);
  if (VEC && i0 + V <= n) {
#pragma unroll
    for (int j = 0; j < V; j += W) {
      const Pack<T, W> q = *reinterpret_cast<const Pack<T, W>*>(p + i0 + j);
#pragma unroll
      for (int l = 0; l < W; ++l) o[j + l] = q.v[l];
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = (i0 + j < n) ? p[i0 + j] : (T)0;
  }
}

template <typename T, int V, bool VEC>
__device__ __forceinline__ void store_chunk(T* __restrict__ p, long long i0, long long n, const T (&o)[V]) {
  if (VEC && i0 + V <= n) {
    Pack<T, V> q;
#pragma unroll
    for (int j = 0; j < V; ++j) q.v[j] = o[j];
    *reinterpret_cast<Pack<T, V>*>(p + i0) = q;
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (i0 + j < n) p[i0 + j] = o[j];
  }
}

// energy, dE/df and Fisher weight of one element (unscaled)
template <int KIND>
__device__ __forceinline__ void lh_terms(double f, double a, double b, bool want_e, bool want_g, double& e,
                                         double& g, double& w) {
#pragma clang fp contract(off)
  if (KIND == NFT_LH_BERNOULLI) {
    // a = d in {0, 1}
    const double omf = 1.0 - f;
    if (want_e) e = -log(f) * a + log(omf) * (a - 1.0);
    if (want_g) g = -a / f + (1.0 - a) / omf;
    w = 1.0 / (f * omf);
  } else if (KIND == NFT_LH_STUDENT_T) {
    // a = theta
    const double f2 = f * f;
    if (want_e) e = ((a + 1.0) / 2.0) * log1p(f2 / a);
    if (want_g) g = (a + 1.0) * f / (a + f2);
    w = (a + 1.0) / (a + 3.0);
  } else {
    // a = alpha + 1, b = beta
    if (want_e) e = a * log(f) + b / f;
    if (want_g) g = a / f - b / (f * f);
    w = a / (f * f);
  }
}

template <typename T, int KIND, bool VEC>
__global__ __launch_bounds__(LH_NT) void lh_eval_kernel(const T* __restrict__ f, const double* __restrict__ p0,
                                                        const double* __restrict__ p1, double c0, long long n,
                                                        long long vs, double scale, double* __restrict__ part,
                                                        T* __restrict__ grad, T* __restrict__ weight) {
#pragma clang fp contract(off)
  constexpr int V = 16 / (int)sizeof(T);
  __shared__ double sh[LH_NT / 64];
  const long long row = blockIdx.y;
  f += row * vs;
  if (grad) grad += row * vs;
  if (weight) weight += row * vs;
  const bool want_e = part != nullptr, want_g = grad != nullptr;
  double acc = 0.0;
  const long long stride = (long long)gridDim.x * LH_NT;
  for (long long c = (long long)blockIdx.x * LH_NT + threadIdx.x; c * V < n; c += stride) {
    const long long i0 = c * V;
    T fv[V], gv[V], wv[V];
    double a[V], b[V];
    load_chunk<T, V, VEC>(f, i0, n, fv);
    if (p0) load_chunk<double, V, VEC>(p0, i0, n, a);
    else {
#pragma unroll
      for (int j = 0; j < V; ++j) a[j] = c0;
    }
    if (KIND == NFT_LH_INVGAMMA) load_chunk<double, V, VEC>(p1, i0, n, b);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      double e = 0.0, g = 0.0, w = 0.0;
      if (i0 + j < n) {
        lh_terms<KIND>((double)fv[j], a[j], KIND == NFT_LH_INVGAMMA ? b[j] : 0.0, want_e, want_g, e, g, w);
        acc += e;
      }
      gv[j] = (T)(g * scale);
      wv[j] = (T)(w * scale);
    }
    if (grad) store_chunk<T, V, VEC>(grad, i0, n, gv);
    if (weight) store_chunk<T, V, VEC>(weight, i0, n, wv);
  }
  if (part) {
    const double s = lh_block_sum(acc, sh);
    if (threadIdx.x == 0) part[row * gridDim.x + blockIdx.x] = s;
  }
}

// value[row] = scale * (fixed-order sum of the row's nb partials)
__global__ __launch_bounds__(LH_NT) void lh_fold_kernel(const double* __restrict__ part, int nb, double scale,
                                                        double* __restrict__ value) {
#pragma clang fp contract(off)
  __shared__ double sh[LH_NT / 64];
  part += (long long)blockIdx.x * nb;
  double v = 0.0;
  for (int b = threadIdx.x; b < nb; b += LH_NT) v += part[b];
  const double s = lh_block_sum(v, sh);
  if (threadIdx.x == 0) value[blockIdx.x] = scale * s;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(LH_NT) void lh_transform_kernel(const T* __restrict__ f, T* __restrict__ t,
                                                             T* __restrict__ dt, long long n) {
#pragma clang fp contract(off)
  constexpr int V = 16 / (int)sizeof(T);
  const long long stride = (long long)gridDim.x * LH_NT;
  for (long long c = (long long)blockIdx.x * LH_NT + threadIdx.x; c * V < n; c += stride) {
    const long long i0 = c * V;
    T fv[V], tv[V], dv[V];
    load_chunk<T, V, VEC>(f, i0, n, fv);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      double tj = 0.0, dj = 0.0;
      if (i0 + j < n) {
        const double x = (double)fv[j], omx = 1.0 - x;
        tj = -2.0 * atan(sqrt(omx / x));
        dj = 1.0 / sqrt(x * omx);
      }
      tv[j] = (T)tj;
      dv[j] = (T)dj;
    }
    store_chunk<T, V, VEC>(t, i0, n, tv);
    store_chunk<T, V, VEC>(dt, i0, n, dv);
  }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <typename T, int KIND>
void launch_eval(bool vec, dim3 grid, hipStream_t s, const void* f, const double* p0, const double* p1, double c0,
                 long long n, long long vs, double scale, double* part, void* grad, void* weight) {
  if (vec)
    hipLaunchKernelGGL((lh_eval_kernel<T, KIND, true>), grid, dim3(LH_NT), 0, s, (const T*)f, p0, p1, c0, n, vs, scale,
                       part, (T*)grad, (T*)weight);
  else
    hipLaunchKernelGGL((lh_eval_kernel<T, KIND, false>), grid, dim3(LH_NT), 0, s, (const T*)f, p0, p1, c0, n, vs,
                       scale, part, (T*)grad, (T*)weight);
}

template <typename T>
void launch_eval_kind(int kind, bool vec, dim3 grid, hipStream_t s, const void* f, const double* p0,
                      const double* p1, double c0, long long n, long long vs, double scale, double* part,
                      void* grad, void* weight) {
  if (kind == NFT_LH_BERNOULLI)
    launch_eval<T, NFT_LH_BERNOULLI>(vec, grid, s, f, p0, p1, c0, n, vs, scale, part, grad, weight);
  else if (kind == NFT_LH_STUDENT_T)
    launch_eval<T, NFT_LH_STUDENT_T>(vec, grid, s, f, p0, p1, c0, n, vs, scale, part, grad, weight);
  else
    launch_eval<T, NFT_LH_INVGAMMA>(vec, grid, s, f, p0, p1, c0, n, vs, scale, part, grad, weight);
}

}  // namespace
}  // namespace nft

using namespace nft;

extern "C" {

int nft_lh_transform_pair(int kind, const void* f, void* t, void* dt, int64_t n, int dtype, hipStream_t stream) {
  if (kind != NFT_LH_BERNOULLI) {
    set_last_error("nft_lh_transform_pair: unknown kind %d", kind);
    return NFT_ERR_ARG;
  }
  if (n < 0 || (n > 0 && (!f || !t || !dt))) {
    set_last_error("nft_lh_transform_pair: bad arguments");
    return NFT_ERR_ARG;
  }
  if (n == 0) return NFT_OK;
  if (dtype != 0 && dtype != 1) {
    set_last_error("nft_lh_transform_pair: bad dtype %d", dtype);
    return NFT_ERR_ARG;
  }
  const int V = dtype == 0 ? 2 : 4;
  const long long chunks = ((long long)n + V - 1) / V;
  const unsigned nb = (unsigned)std::min<long long>((chunks + LH_NT - 1) / LH_NT, 65536);
  const bool vec = al16(f) && al16(t) && al16(dt);
  prof_mark(stream, "lh_transform_pair");
  if (dtype == 0) {
    if (vec)
      hipLaunchKernelGGL((lh_transform_kernel<double, true>), dim3(nb), dim3(LH_NT), 0, stream, (const double*)f,
                         (double*)t, (double*)dt, (long long)n);
    else
      hipLaunchKernelGGL((lh_transform_kernel<double, false>), dim3(nb), dim3(LH_NT), 0, stream, (const double*)f,
                         (double*)t, (double*)dt, (long long)n);
  } else {
    if (vec)
      hipLaunchKernelGGL((lh_transform_kernel<float, true>), dim3(nb), dim3(LH_NT), 0, stream, (const float*)f,
                         (float*)t, (float*)dt, (long long)n);
    else
      hipLaunchKernelGGL((lh_transform_kernel<float, false>), dim3(nb), dim3(LH_NT), 0, stream, (const float*)f,
                         (float*)t, (float*)dt, (long long)n);
  }
  NFT_HIP_CHECK(hipGetLastError());
  return NFT_OK;
}

int nft_lh_eval_batched(int kind, const void* f, const double* p0, const double* p1, double c0, int64_t n,
                        int64_t vstride, int nrhs, int dtype, double scale, double* value, void* grad,
                        void* weight, void* ws, hipStream_t stream) {
  if (kind != NFT_LH_BERNOULLI && kind != NFT_LH_STUDENT_T && kind != NFT_LH_INVGAMMA) {
    set_last_error("nft_lh_eval_batched: unknown kind %d", kind);
    return NFT_ERR_ARG;
  }
  if (dtype != 0 && dtype != 1) {
    set_last_error("nft_lh_eval_batched: bad dtype %d", dtype);
    return NFT_ERR_ARG;
  }
  if (n < 0 || nrhs < 1 || vstride < n) {
    set_last_error("nft_lh_eval_batched: bad sizes (n %lld, nrhs %d, vstride %lld)", (long long)n, nrhs,
                   (long long)vstride);
    return NFT_ERR_ARG;
  }
  if (n > 0 && !f) {
    set_last_error("nft_lh_eval_batched: f is NULL");
    return NFT_ERR_ARG;
  }
  if (n > 0 && ((kind != NFT_LH_STUDENT_T && !p0) || (kind == NFT_LH_INVGAMMA && !p1))) {
    set_last_error("nft_lh_eval_batched: kind %d lacks a parameter array", kind);
    return NFT_ERR_ARG;
  }
  if (value && !ws) {
    set_last_error("nft_lh_eval_batched: value needs a workspace");
    return NFT_ERR_ARG;
  }
  if (!value && !grad && !weight) return NFT_OK;
  // as many workgroups per row as nft_reduce_workspace(n) holds partials for
  const int nb = (int)(nft_reduce_workspace(n) / (3 * sizeof(double)));
  double* part = value ? (double*)ws : nullptr;
  if (n > 0) {
    const size_t es = dtype == 0 ? 8 : 4;
    const bool rows_al = nrhs == 1 || (vstride * es) % 16 == 0;
    const bool vec = rows_al && al16(f) && al16(p0) && al16(p1) && al16(grad) && al16(weight);
    const dim3 grid(nb, nrhs);
    prof_mark(stream, "lh_eval");
    if (dtype == 0)
      launch_eval_kind<double>(kind, vec, grid, stream, f, p0, p1, c0, (long long)n, (long long)vstride, scale, part,
                               grad, weight);
    else
      launch_eval_kind<float>(kind, vec, grid, stream, f, p0, p1, c0, (long long)n, (long long)vstride, scale, part,
                              grad, weight);
  }
  if (value) {
    // n == 0: no partials were written, the energy of an empty row is 0
    prof_mark(stream, "lh_fold");
    hipLaunchKernelGGL(lh_fold_kernel, dim3(nrhs), dim3(LH_NT), 0, stream, part, n > 0 ? nb : 0, scale, value);
  }
  NFT_HIP_CHECK(hipGetLastError());
  return NFT_OK;
}

}  // extern "C"
