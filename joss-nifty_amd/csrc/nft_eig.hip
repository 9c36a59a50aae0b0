// Tall-skinny Gram kernels of the block-Lanczos eigen-solver
// (minimization/block_lanczos.py): the orthogonalisation of a block of k <= 8
// vectors against a basis of m vectors, both of n elements,
//
//   nft_gram_dots   C[j, b] = V_j . W_b                      (V^T W)
//   nft_gram_axpy   W_b = beta W_b + sum_j T[j, b] V_j       (W -= V C, Ritz vectors)
//
// Replaces what the reference leaves to ARPACK's dsaupd on the host
// (src/evidence_lower_bound.py:93, one matvec at a time) and its _Projector
// (src/evidence_lower_bound.py:49-53).
//
// A workgroup of 256 threads owns a tile of GRAM_TILE = 2048 elements and
// keeps that tile of the k block rows in registers (8 elements per thread and
// row); the m basis rows stream through it, each element of V read once per
// call.  fp64 only, wave64, no atomics, no device-global state.  Sums are
// fixed-order: per thread an fma chain over its 8 elements in index order,
// the wave64 shuffle tree, the 4 wave sums in order, then a second kernel
// folds the per-tile partials in tile order (the two-level fold of
// nft_blas.hip).  A row's result depends neither on k nor on the row's place
// in the block: every (j, b) runs the same instructions on its own operands.
//
// Loads are 16-byte where the base pointers are 16-byte aligned and the row
// strides (of operands with more than one row) even, and 8-byte otherwise;
// which thread owns which element is the same in both cases, so the summation
// order is too.
#include "nft_api_internal.hpp"
#include "../../include/nifty_amd.h"

namespace nft {

constexpr int GRAM_NT = 256;
constexpr int GRAM_EPT = 8;                    // elements per thread and row
constexpr int GRAM_TILE = GRAM_NT * GRAM_EPT;  // 2048
constexpr int GRAM_KMAX = 8;

static long long gram_blocks(long long n) { return n < 1 ? 0 : (n + GRAM_TILE - 1) / GRAM_TILE; }

__device__ __forceinline__ double gram_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// the thread's 8 elements of one row: pairs (i0 + p * 512 + {0, 1}), p < 4,
// with i0 = tile start + 2 * thread; elements at or beyond n read as zero
template <bool VEC>
__device__ __forceinline__ void gram_load(const double* __restrict__ row, long long i0, long long n,
                                          double (&x)[GRAM_EPT]) {
#pragma unroll
  for (int p = 0; p < GRAM_EPT / 2; ++p) {
    const long long i = i0 + (long long)p * (2 * GRAM_NT);
    if (VEC && i + 1 < n) {
      const double2 t = *reinterpret_cast<const double2*>(row + i);
      x[2 * p] = t.x;
      x[2 * p + 1] = t.y;
    } else {
      x[2 * p] = i < n ? row[i] : 0.0;
      x[2 * p + 1] = i + 1 < n ? row[i + 1] : 0.0;
    }
  }
}

template <bool VEC>
__device__ __forceinline__ void gram_store(double* __restrict__ row, long long i0, long long n,
                                           const double (&x)[GRAM_EPT]) {
#pragma unroll
  for (int p = 0; p < GRAM_EPT / 2; ++p) {
    const long long i = i0 + (long long)p * (2 * GRAM_NT);
    if (VEC && i + 1 < n) {
      *reinterpret_cast<double2*>(row + i) = make_double2(x[2 * p], x[2 * p + 1]);
    } else {
      if (i < n) row[i] = x[2 * p];
      if (i + 1 < n) row[i + 1] = x[2 * p + 1];
    }
  }
}

// part[(j * K + b) * nb + tile] = the tile's share of V_j . W_b
template <int K, bool VEC>
__global__ __launch_bounds__(GRAM_NT) void gram_dots_kernel(const double* __restrict__ V, long long vstride, int m,
                                                            const double* __restrict__ W, long long wstride,
                                                            long long n, double* __restrict__ part) {
  __shared__ double sh[2][GRAM_KMAX][GRAM_NT / 64];
  const long long nb = gridDim.x;
  const long long i0 = (long long)blockIdx.x * GRAM_TILE + 2 * threadIdx.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  double w[K][GRAM_EPT];
#pragma unroll
  for (int b = 0; b < K; ++b) gram_load<VEC>(W + b * wstride, i0, n, w[b]);
  double v[GRAM_EPT];
  gram_load<VEC>(V, i0, n, v);
  for (int j = 0; j < m; ++j) {
    // the next basis row's loads are in flight while this one is reduced
    double vn[GRAM_EPT];
    if (j + 1 < m) gram_load<VEC>(V + (long long)(j + 1) * vstride, i0, n, vn);
    double (*s)[GRAM_NT / 64] = sh[j & 1];
#pragma unroll
    for (int b = 0; b < K; ++b) {
      double a = 0.0;
#pragma unroll
      for (int e = 0; e < GRAM_EPT; ++e) a = fma(v[e], w[b][e], a);
      a = gram_wave_sum(a);
      if (lane == 0) s[b][wid] = a;
    }
    // double-buffered: the writes of row j + 2 come after the barrier of row
    // j + 1, which every thread passes only after the reads of row j
    __syncthreads();
    if (threadIdx.x < K) {
      const int b = threadIdx.x;
      double t = 0.0;
#pragma unroll
      for (int q = 0; q < GRAM_NT / 64; ++q) t += s[b][q];
      part[((long long)j * K + b) * nb + blockIdx.x] = t;
    }
    if (j + 1 < m) {
#pragma unroll
      for (int e = 0; e < GRAM_EPT; ++e) v[e] = vn[e];
    }
  }
}

// C[r] = sum of part[r * nb + t] over the tiles t: thread-strided sums in
// tile order, the wave tree, the 4 wave sums in order
__global__ __launch_bounds__(GRAM_NT) void gram_fold_kernel(const double* __restrict__ part, long long nb,
                                                            double* __restrict__ C) {
  __shared__ double sh[GRAM_NT / 64];
  part += (long long)blockIdx.x * nb;
  double v = 0.0;
  for (long long t = threadIdx.x; t < nb; t += GRAM_NT) v += part[t];
  v = gram_wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < GRAM_NT / 64; ++q) t += sh[q];
    C[blockIdx.x] = t;
  }
}

// W_b = beta W_b + sum_j T[j * K + b] V_j, j ascending, one fma per term
template <int K, bool VEC>
__global__ __launch_bounds__(GRAM_NT) void gram_axpy_kernel(const double* __restrict__ V, long long vstride, int m,
                                                            const double* __restrict__ T, double* __restrict__ W,
                                                            long long wstride, long long n, int keep) {
  const long long i0 = (long long)blockIdx.x * GRAM_TILE + 2 * threadIdx.x;
  double w[K][GRAM_EPT];
#pragma unroll
  for (int b = 0; b < K; ++b) {
    if (keep) {
      gram_load<VEC>(W + b * wstride, i0, n, w[b]);
    } else {
#pragma unroll
      for (int e = 0; e < GRAM_EPT; ++e) w[b][e] = 0.0;
    }
  }
#pragma unroll 2
  for (int j = 0; j < m; ++j) {
    double v[GRAM_EPT];
    gram_load<VEC>(V + (long long)j * vstride, i0, n, v);
#pragma unroll
    for (int b = 0; b < K; ++b) {
      const double t = T[(long long)j * K + b];
#pragma unroll
      for (int e = 0; e < GRAM_EPT; ++e) w[b][e] = fma(t, v[e], w[b][e]);
    }
  }
#pragma unroll
  for (int b = 0; b < K; ++b) gram_store<VEC>(W + b * wstride, i0, n, w[b]);
}

// a stride counts only where there is a second row to reach with it
static bool gram_vec_ok(const void* V, long long vstride, int m, const void* W, long long wstride, int k) {
  return (((uintptr_t)V | (uintptr_t)W) & 15) == 0 && (m == 1 || (vstride & 1) == 0) &&
         (k == 1 || (wstride & 1) == 0);
}

// the argument checks shared by both entry points (before any launch)
static int gram_check(const char* who, const void* V, long long vstride, int m, const void* W, long long wstride,
                      int k, long long n, int dtype) {
  if (dtype != 0) {
    set_last_error("%s: fp64 only (dtype %d)", who, dtype);
    return NFT_ERR_ARG;
  }
  if (!V || !W || m < 1 || k < 1 || k > GRAM_KMAX || n < 1 || (m > 1 && vstride < n) || (k > 1 && wstride < n)) {
    set_last_error("%s: bad arguments (m %d, k %d, n %lld, vstride %lld, wstride %lld)", who, m, k, n, vstride,
                   wstride);
    return NFT_ERR_ARG;
  }
  if (gram_blocks(n) > 0x7fffffffLL) {
    set_last_error("%s: n %lld too long", who, n);
    return NFT_ERR_ARG;
  }
  return NFT_OK;
}

template <int K>
static void launch_dots(bool vec, unsigned nb, hipStream_t s, const double* V, long long vstride, int m,
                        const double* W, long long wstride, long long n, double* part) {
  if (vec)
    hipLaunchKernelGGL((gram_dots_kernel<K, true>), dim3(nb), dim3(GRAM_NT), 0, s, V, vstride, m, W, wstride, n,
                       part);
  else
    hipLaunchKernelGGL((gram_dots_kernel<K, false>), dim3(nb), dim3(GRAM_NT), 0, s, V, vstride, m, W, wstride, n,
                       part);
}

template <int K>
static void launch_axpy(bool vec, unsigned nb, hipStream_t s, const double* V, long long vstride, int m,
                        const double* T, double* W, long long wstride, long long n, int keep) {
  if (vec)
    hipLaunchKernelGGL((gram_axpy_kernel<K, true>), dim3(nb), dim3(GRAM_NT), 0, s, V, vstride, m, T, W, wstride, n,
                       keep);
  else
    hipLaunchKernelGGL((gram_axpy_kernel<K, false>), dim3(nb), dim3(GRAM_NT), 0, s, V, vstride, m, T, W, wstride, n,
                       keep);
}

}  // namespace nft

using namespace nft;

#define GRAM_DISPATCH_K(k, CALL) \
  switch (k) {                   \
    case 1: CALL(1); break;      \
    case 2: CALL(2); break;      \
    case 3: CALL(3); break;      \
    case 4: CALL(4); break;      \
    case 5: CALL(5); break;      \
    case 6: CALL(6); break;      \
    case 7: CALL(7); break;      \
    default: CALL(8); break;     \
  }

extern "C" {

int nft_gram_tile(void) { return GRAM_TILE; }

int nft_gram_blocks(int64_t n) {
  const long long b = gram_blocks(n);
  return b > 0x7fffffffLL ? 0 : (int)b;
}

size_t nft_gram_workspace(int m, int k, int64_t n) {
  if (m < 1 || k < 1 || n < 1) return 0;
  return (size_t)m * (size_t)k * (size_t)gram_blocks(n) * sizeof(double);
}

int nft_gram_dots(const void* V, int64_t vstride, int m, const void* W, int64_t wstride, int k, int64_t n, int dtype,
                  double* C, void* ws, size_t ws_bytes, hipStream_t stream) {
  const int st = gram_check("nft_gram_dots", V, vstride, m, W, wstride, k, n, dtype);
  if (st != NFT_OK) return st;
  if (!C || !ws || ws_bytes < nft_gram_workspace(m, k, n)) {
    set_last_error("nft_gram_dots: NULL result or workspace below nft_gram_workspace(m, k, n)");
    return NFT_ERR_ARG;
  }
  const unsigned nb = (unsigned)gram_blocks(n);
  const bool vec = gram_vec_ok(V, vstride, m, W, wstride, k);
  double* part = (double*)ws;
  prof_mark(stream, "gram_dots");
#define CALL(K) \
  launch_dots<K>(vec, nb, stream, (const double*)V, (long long)vstride, m, (const double*)W, (long long)wstride, \
                 (long long)n, part)
  GRAM_DISPATCH_K(k, CALL)
#undef CALL
  prof_mark(stream, "gram_fold");
  hipLaunchKernelGGL(gram_fold_kernel, dim3((unsigned)(m * k)), dim3(GRAM_NT), 0, stream, part, (long long)nb, C);
  NFT_HIP_CHECK(hipGetLastError());
  return NFT_OK;
}

int nft_gram_axpy(const void* V, int64_t vstride, int m, const double* T, void* W, int64_t wstride, int k, int64_t n,
                  int dtype, double beta, hipStream_t stream) {
  const int st = gram_check("nft_gram_axpy", V, vstride, m, W, wstride, k, n, dtype);
  if (st != NFT_OK) return st;
  if (!T || (beta != 0.0 && beta != 1.0)) {
    set_last_error("nft_gram_axpy: NULL coefficients or beta %g (0 or 1)", beta);
    return NFT_ERR_ARG;
  }
  // W may not alias V: the spans [V, V_{m-1} + n) and [W, W_{k-1} + n)
  const uintptr_t v0 = (uintptr_t)V, v1 = v0 + ((uintptr_t)(m - 1) * (uintptr_t)vstride + (uintptr_t)n) * 8;
  const uintptr_t w0 = (uintptr_t)W, w1 = w0 + ((uintptr_t)(k - 1) * (uintptr_t)wstride + (uintptr_t)n) * 8;
  if (v0 < w1 && w0 < v1) {
    set_last_error("nft_gram_axpy: W aliases V");
    return NFT_ERR_ARG;
  }
  const unsigned nb = (unsigned)gram_blocks(n);
  const bool vec = gram_vec_ok(V, vstride, m, W, wstride, k);
  prof_mark(stream, "gram_axpy");
#define CALL(K) \
  launch_axpy<K>(vec, nb, stream, (const double*)V, (long long)vstride, m, T, (double*)W, (long long)wstride, \
                 (long long)n, beta != 0.0 ? 1 : 0)
  GRAM_DISPATCH_K(k, CALL)
#undef CALL
  NFT_HIP_CHECK(hipGetLastError());
  return NFT_OK;
}

}  // extern "C"
