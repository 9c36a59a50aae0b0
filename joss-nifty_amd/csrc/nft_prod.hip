// Product-spectrum correlated fields (two add_fluctuations components of the
// CorrelatedFieldMaker on a product domain, src/library/correlated_fields.py:
// 764-823) on the one-space fused engine.
//
// 1. nft_mirror_mix: y = R x with R = (P1 + P2 + I - P1 P2) / 2, P_g the point
//    mirror k -> -k on the grid axes of group g.  R is symmetric, orthogonal
//    and an involution, and H_1 (x) H_2 = R H_joint = H_joint R: in the frame
//    xi' = R xi the product field is a one-space field on the joint grid.
//    A thread owns a whole orbit {k, P1 k, P2 k, P1 P2 k} (degenerate ones
//    included): it loads the orbit, then stores it, so the pass works in place
//    and moves every element once in and once out.  Neighbouring lanes hold
//    neighbouring k, so the mirrored accesses are contiguous runs in reverse
//    lane order (whole lines, no strided loads).
//
// 2. The amplitude table over the combined bins b = b1 * B2 + b2,
//      A[0,0] = z   A[b1,0] = a1[b1]   A[0,b2] = a2[b2]   A[b1,b2] = a1 a2 / z,
//    a_i = s_i m_i the components' amplitudes (m_i as the nft_amp kernels give
//    them, entry 0 ignored), z = s_0 exp(lm_o + ls_o x_zm), with its JVP (one
//    streaming pass) and VJP (tile partials + fixed-order fold).
//
// fp64 (the mix also fp32), wave64, no atomics, no device-global state.
#include "nft_common.hpp"

namespace nft {

constexpr int PT = 256;   // threads per workgroup: 4 waves of 64
constexpr int PRB = 16;   // VJP tile: PRB rows (b1) x PT columns (b2)

static inline long long pblk(long long n, long long t) { return (n + t - 1) / t; }
static inline long long peven(long long n) { return (n + 1) & ~1LL; }

__device__ __forceinline__ bool pal16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ------------------------------------------------------------- mirror mix
// grid (n0, n1, n2) (leading axes of length 1 for fewer than 3), axes [0, sp)
// in group 1, [sp, 3) in group 2; row = blockIdx.y
template <typename T>
__global__ __launch_bounds__(PT) void mirror_mix(const T* x, long long xs, T* y, long long ys, long long n0,
                                                 long long n1, long long n2, int sp) {
  const long long N = n0 * n1 * n2;
  const long long f = (long long)blockIdx.x * PT + threadIdx.x;
  if (f >= N) return;
  const long long i2 = f % n2, q = f / n2, i1 = q % n1, i0 = q / n1;
  const long long j0 = i0 ? n0 - i0 : 0, j1 = i1 ? n1 - i1 : 0, j2 = i2 ? n2 - i2 : 0;
  // the axes' mirrors by group (axis 0 is always in group 1, axis 2 in group 2)
  const long long b1 = sp >= 2 ? j1 : i1, c1 = sp >= 2 ? i1 : j1;
  const long long ob = (j0 * n1 + b1) * n2 + i2;   // P1 k
  const long long oc = (i0 * n1 + c1) * n2 + j2;   // P2 k
  if (ob < f || oc < f) return;                    // the orbit's first point owns it
  const long long od = (j0 * n1 + j1) * n2 + j2;   // P1 P2 k
  const bool e1 = ob == f, e2 = oc == f;
  const T* xr = x + (long long)blockIdx.y * xs;
  T* yr = y + (long long)blockIdx.y * ys;
  const T a = xr[f];
  const T b = e1 ? a : xr[ob];
  const T c = e2 ? a : xr[oc];
  const T d = e1 ? c : e2 ? b : xr[od];
  const T h = (T)0.5;
  yr[f] = ((a + b) + c - d) * h;
  if (!e1) yr[ob] = ((b + a) + d - c) * h;
  if (!e2) yr[oc] = ((c + d) + a - b) * h;
  if (!e1 && !e2) yr[od] = ((d + c) + b - a) * h;
}

// ------------------------------------------------------------------ table
// the constants of one linearisation, doubles: [0] z, [1] z ls_o,
// [2 ..) p1 = a1 / z (B1 values, entry 0 = 0), then from 2 + even(B1):
// p2 = a2 / z (B2 values, entry 0 = 0)
struct PDims {
  long long B1, B2;
  __host__ __device__ long long o2() const { return 2 + ((B1 + 1) & ~1LL); }
};

__global__ __launch_bounds__(PT) void prod_fwd(PDims dm, const double* m1, long long m1s, const double* m2,
                                               long long m2s, const double* xz, long long ls, double lm_o,
                                               double ls_o, double s0, double s1, double s2, double* A,
                                               long long As, double* cb, long long cbs) {
  const int r = blockIdx.y;
  const long long b = (long long)blockIdx.x * PT + threadIdx.x;
  if (b >= dm.B1 * dm.B2) return;
  const long long b1 = b / dm.B2, b2 = b % dm.B2;
  const double z = s0 * exp(lm_o + ls_o * xz[r * ls]);
  const double a1 = b1 ? s1 * m1[r * m1s + b1] : 0.0;
  const double a2 = b2 ? s2 * m2[r * m2s + b2] : 0.0;
  double* c = cb + r * cbs;
  double v;
  if (b1 == 0) {
    v = b2 ? a2 : z;
    c[dm.o2() + b2] = b2 ? a2 / z : 0.0;
    if (b2 == 0) c[0] = z, c[1] = z * ls_o, c[2] = 0.0;
  } else if (b2 == 0) {
    v = a1;
    c[2 + b1] = a1 / z;
  } else {
    v = (a1 * a2) / z;
  }
  A[r * As + b] = v;
}

// one entry of the table tangent: the same expression for any batch size
__device__ __forceinline__ double pjv(const double* c, PDims dm, long long b, double d1, double d2, double dz) {
  const long long b1 = b / dm.B2, b2 = b % dm.B2;
  if (b1 == 0) return b2 ? d2 : dz;
  if (b2 == 0) return d1;
  const double p1 = c[2 + b1], p2 = c[dm.o2() + b2];
  return fma(d1, p2, fma(p1, d2, -(p1 * p2) * dz));
}

// da[b * k + r], bin-major; a thread owns two consecutive values
__global__ __launch_bounds__(PT) void prod_jvp(PDims dm, const double* c, double s1, double s2, const double* d1,
                                               long long d1s, const double* d2, long long d2s, const double* tz,
                                               long long ls, double* da, int k) {
  const long long tot = dm.B1 * dm.B2 * k;
  const long long f0 = 2 * ((long long)blockIdx.x * PT + threadIdx.x);
  if (f0 >= tot) return;
  const double gz = c[1];
  double v[2] = {0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long long f = f0 + i;
    if (f >= tot) break;
    const long long b = f / k;
    const int r = (int)(f % k);
    const long long b1 = b / dm.B2, b2 = b % dm.B2;
    v[i] = pjv(c, dm, b, s1 * d1[r * d1s + b1], s2 * d2[r * d2s + b2], gz * tz[r * ls]);
  }
  if (f0 + 1 < tot && pal16(da + f0)) {
    *reinterpret_cast<double2*>(da + f0) = make_double2(v[0], v[1]);
  } else {
    da[f0] = v[0];
    if (f0 + 1 < tot) da[f0 + 1] = v[1];
  }
}

// workspace of one right-hand side, doubles: row partials [ntj][B1], column
// partials [nti][B2], full partials [nti * ntj]
struct PWs {
  long long nti, ntj, orow, ocol, ofull, size;
  __host__ __device__ PWs(PDims dm) {
    nti = (dm.B1 + PRB - 1) / PRB, ntj = (dm.B2 + PT - 1) / PT;
    orow = 0, ocol = ntj * dm.B1, ofull = ocol + nti * dm.B2;
    size = (ofull + nti * ntj + 1) & ~1LL;
  }
};

// tile (blockIdx.y, blockIdx.x) of right-hand side blockIdx.z: thread t holds
// column b2 = blockIdx.x * PT + t of the tile's PRB rows
__global__ __launch_bounds__(PT) void prod_vjp_part(PDims dm, const double* c, const double* g, long long gs,
                                                    double* ws) {
  __shared__ double red[PRB + 1][PT / 64];
  const PWs w(dm);
  const int r = blockIdx.z;
  const long long b2 = (long long)blockIdx.x * PT + threadIdx.x, r0 = (long long)blockIdx.y * PRB;
  const bool cv = b2 < dm.B2;
  const double p2 = cv && b2 ? c[dm.o2() + b2] : 0.0, w2 = b2 ? p2 : 1.0;
  const double* gr = g + r * gs;
  double* wr = ws + r * w.size;
  double rowv[PRB], col = 0.0, full = 0.0;
#pragma unroll
  for (int i = 0; i < PRB; ++i) {
    const long long b1 = r0 + i;
    const bool ok = cv && b1 < dm.B1;
    const double v = ok ? gr[b1 * dm.B2 + b2] : 0.0;
    const double p1 = ok && b1 ? c[2 + b1] : 0.0;
    rowv[i] = v * w2;
    col = fma(v, b1 ? p1 : 1.0, col);
    full = fma(v * p1, p2, full);
  }
  if (cv) wr[w.ocol + blockIdx.y * dm.B2 + b2] = col;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i <= PRB; ++i) {
    double s = i < PRB ? rowv[i] : full;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) red[i][wave] = s;
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t > PRB) return;
  const double s = ((red[t][0] + red[t][1]) + red[t][2]) + red[t][3];
  if (t == PRB)
    wr[w.ofull + blockIdx.y * w.ntj + blockIdx.x] = s;
  else if (r0 + t < dm.B1)
    wr[w.orow + blockIdx.x * dm.B1 + r0 + t] = s;
}

// the fold of right-hand side blockIdx.y: the waves of workgroups [0, nbo) sum
// the row / column partials of one output each, workgroup nbo the full
// partials (thread t the partials t, t + PT, ... in order, then the wave sums)
__global__ __launch_bounds__(PT) void prod_vjp_fold(PDims dm, const double* c, double s1, double s2,
                                                    const double* g, long long gs, const double* ws, double* g1,
                                                    long long g1s, double* g2, long long g2s, double* oz,
                                                    const double* dz, long long ls, double shift, int nbo) {
  __shared__ double red[PT / 64];
  const PWs w(dm);
  const int r = blockIdx.y;
  const double* wr = ws + r * w.size;
  const int lane = threadIdx.x & 63;
  if ((int)blockIdx.x < nbo) {
    // one wave per output: lane l sums the tiles l, l + 64, ... in order
    const long long j = (long long)blockIdx.x * (PT / 64) + (threadIdx.x >> 6);
    if (j >= dm.B1 + dm.B2) return;
    const bool row = j < dm.B1;
    const long long i = row ? j : j - dm.B1, nt = row ? w.ntj : w.nti, ld = row ? dm.B1 : dm.B2;
    const double* p = wr + (row ? w.orow : w.ocol) + i;
    double s = 0.0;
    for (long long t = lane; t < nt; t += 64) s += p[t * ld];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) {
      if (row)
        g1[r * g1s + i] = i ? s1 * s : 0.0;
      else
        g2[r * g2s + i] = i ? s2 * s : 0.0;
    }
    return;
  }
  double s = 0.0;
  for (long long i = threadIdx.x; i < w.nti * w.ntj; i += PT) s += wr[w.ofull + i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x) return;
  s = ((red[0] + red[1]) + red[2]) + red[3];
  const double v = c[1] * (g[r * gs] - s);
  oz[r * ls] = dz ? fma(shift, dz[r * ls], v) : v;
}

static bool pdims_ok(int64_t B1, int64_t B2) {
  return B1 >= 2 && B2 >= 2 && B1 <= (int64_t)1 << 31 && B2 <= (int64_t)1 << 31 && B1 * B2 < (int64_t)1 << 40;
}

}  // namespace nft

using namespace nft;

extern "C" {

int nft_mirror_mix(const void* x, int64_t x_stride, void* y, int64_t y_stride, int nrow, int ndim,
                   const int64_t* shape, int split, int dtype, hipStream_t s) {
  bool ok = x && y && shape && nrow >= 1 && nrow <= 65535 && ndim >= 2 && ndim <= 3 && split >= 1 && split < ndim &&
            (dtype == 0 || dtype == 1) && x_stride >= 0 && y_stride >= 0;
  long long n[3] = {1, 1, 1}, N = 1;
  if (ok)
    for (int i = 0; i < ndim; ++i) {
      n[3 - ndim + i] = shape[i];
      if (shape[i] < 1 || shape[i] >= (int64_t)1 << 31) ok = false;
      N *= shape[i] > 0 ? shape[i] : 1;
    }
  if (ok && (N >= (long long)1 << 40 || (nrow > 1 && (y_stride < N || x_stride < N)) || (x == y && x_stride != y_stride)))
    ok = false;
  if (!ok) {
    set_last_error("nft_mirror_mix: invalid arguments (2..3 axes of length >= 1, 1 <= split < ndim, nrow >= 1, "
                   "strides >= the grid size for nrow > 1, equal strides in place, dtype 0 | 1)");
    return NFT_ERR_ARG;
  }
  const int sp = split + (3 - ndim);
  const dim3 grid((unsigned)pblk(N, PT), (unsigned)nrow);
  prof_mark(s, "mirror_mix");
  if (dtype == 0)
    hipLaunchKernelGGL(mirror_mix<double>, grid, dim3(PT), 0, s, (const double*)x, (long long)x_stride, (double*)y,
                       (long long)y_stride, n[0], n[1], n[2], sp);
  else
    hipLaunchKernelGGL(mirror_mix<float>, grid, dim3(PT), 0, s, (const float*)x, (long long)x_stride, (float*)y,
                       (long long)y_stride, n[0], n[1], n[2], sp);
  NFT_HIP_CHECK(hipGetLastError());
  return NFT_OK;
}

int64_t nft_prod_const_size(int64_t B1, int64_t B2) {
  return pdims_ok(B1, B2) ? 2 + peven(B1) + peven(B2) : 0;
}

size_t nft_prod_workspace(int64_t B1, int64_t B2) {
  if (!pdims_ok(B1, B2)) return 0;
  return (size_t)PWs(PDims{B1, B2}).size * sizeof(double);
}

int nft_prod_forward(int64_t B1, int64_t B2, const double* m1, int64_t m1_stride, const double* m2,
                     int64_t m2_stride, const double* x_zm, int64_t lat_stride, double lm_o, double ls_o, double s0,
                     double s1, double s2, int nitem, double* A, int64_t A_stride, double* consts,
                     int64_t const_stride, hipStream_t s) {
  if (!pdims_ok(B1, B2) || !m1 || !m2 || !x_zm || !A || !consts || nitem < 1 || nitem > 65535 || m1_stride < 0 ||
      m2_stride < 0 || lat_stride < 0 || !(s0 > 0.0) ||
      (nitem > 1 && (A_stride < B1 * B2 || const_stride < nft_prod_const_size(B1, B2)))) {
    set_last_error("nft_prod_forward: invalid arguments (B1, B2 >= 2, nitem >= 1, non-null pointers, s0 > 0, "
                   "output rows that do not overlap)");
    return NFT_ERR_ARG;
  }
  prof_mark(s, "prod_fwd");
  hipLaunchKernelGGL(prod_fwd, dim3((unsigned)pblk(B1 * B2, PT), (unsigned)nitem), dim3(PT), 0, s, PDims{B1, B2}, m1,
                     (long long)m1_stride, m2, (long long)m2_stride, x_zm, (long long)lat_stride, lm_o, ls_o, s0, s1,
                     s2, A, (long long)A_stride, consts, (long long)const_stride);
  NFT_HIP_CHECK(hipGetLastError());
  return NFT_OK;
}

int nft_prod_jvp_batched(int64_t B1, int64_t B2, const double* consts, double s1, double s2, const double* dm1,
                         int64_t dm1_stride, const double* dm2, int64_t dm2_stride, const double* t_zm,
                         int64_t lat_stride, double* da, int nrhs, hipStream_t s) {
  if (!pdims_ok(B1, B2) || !consts || !dm1 || !dm2 || !t_zm || !da || nrhs < 1 || nrhs > 4096 || lat_stride < 0 ||
      dm1_stride < (nrhs > 1 ? B1 : 0) || dm2_stride < (nrhs > 1 ? B2 : 0)) {
    set_last_error("nft_prod_jvp_batched: invalid arguments (B1, B2 >= 2, 1 <= nrhs <= 4096, non-null pointers, "
                   "dm rows that do not overlap)");
    return NFT_ERR_ARG;
  }
  prof_mark(s, "prod_jvp");
  hipLaunchKernelGGL(prod_jvp, dim3((unsigned)pblk(B1 * B2 * nrhs, 2 * PT)), dim3(PT), 0, s, PDims{B1, B2}, consts, s1,
                     s2, dm1, (long long)dm1_stride, dm2, (long long)dm2_stride, t_zm, (long long)lat_stride, da,
                     nrhs);
  NFT_HIP_CHECK(hipGetLastError());
  return NFT_OK;
}

int nft_prod_vjp_batched(int64_t B1, int64_t B2, const double* consts, double s1, double s2, const double* g,
                         int64_t g_stride, double* gm1, int64_t gm1_stride, double* gm2, int64_t gm2_stride,
                         double* out_zm, const double* d_zm, int64_t lat_stride, double shift, double* ws, int nrhs,
                         hipStream_t s) {
  bool ok = pdims_ok(B1, B2) && consts && g && gm1 && gm2 && out_zm && ws && nrhs >= 1 && nrhs <= 65535 &&
            lat_stride >= 0 && g_stride >= 0;
  if (ok && nrhs > 1 && (g_stride < B1 * B2 || gm1_stride < B1 || gm2_stride < B2 || lat_stride < 1)) ok = false;
  const PDims dm{B1, B2};
  const PWs w(dm);
  if (ok && (w.nti > 65535 || w.ntj > 0x7fffffffLL)) ok = false;
  if (!ok) {
    set_last_error("nft_prod_vjp_batched: invalid arguments (B1, B2 >= 2, nrhs >= 1, non-null pointers, rows of "
                   "g, gm1, gm2 and out_zm that do not overlap for nrhs > 1)");
    return NFT_ERR_ARG;
  }
  const double* dz = (d_zm && shift != 0.0) ? d_zm : nullptr;
  prof_mark(s, "prod_vjp_part");
  hipLaunchKernelGGL(prod_vjp_part, dim3((unsigned)w.ntj, (unsigned)w.nti, (unsigned)nrhs), dim3(PT), 0, s, dm, consts,
                     g, (long long)g_stride, ws);
  const int nbo = (int)pblk(B1 + B2, PT / 64);
  prof_mark(s, "prod_vjp_fold");
  hipLaunchKernelGGL(prod_vjp_fold, dim3((unsigned)nbo + 1, (unsigned)nrhs), dim3(PT), 0, s, dm, consts, s1, s2, g,
                     (long long)g_stride, ws, gm1, (long long)gm1_stride, gm2, (long long)gm2_stride, out_zm, dz,
                     (long long)lat_stride, shift, nbo);
  NFT_HIP_CHECK(hipGetLastError());
  return NFT_OK;
}

}  // extern "C"
