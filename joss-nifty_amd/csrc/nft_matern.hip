// Matern-kernel amplitude of the correlated field
// (src/library/correlated_fields.py:233-274 with the zero-mode and volume
// factors of :360-384, :862-938) and its rank-3 (4 with the zero mode)
// Jacobian, fp64:
//
//   A_0 = V zm                                   (0 without a zero mode)
//   A_b = sqrt(V) s (1 + u_b)^(l/4),  u_b = k_b^2 / c^2,   b >= 1
//
// One linearisation is three finished columns of B values (entry 0 is 0)
//   gs = ls_s A,  gc = -(l ls_c / 2) A u / (1 + u),  gl = (sig_l / 4) A log1p(u)
// plus the scalar gz = V zm ls_o of the zero mode, so the JVP is one
// streaming pass and the VJP three dot products.  Key order everywhere:
// scale, cutoff, loglogslope, zeromode.  No atomics, no device-global state.
#include "nft_common.hpp"
#include <algorithm>

namespace nft {

using MConst = nft_matern_const;
using MModel = nft_matern_model;

constexpr int MT = 256;        // threads per workgroup: 4 waves of 64
constexpr int MTILE = 2 * MT;  // bins per workgroup (two per thread)

static inline int mblk(long long n, int tile) { return (int)((n + tile - 1) / tile); }

__device__ __forceinline__ bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

struct MCols {
  const double *gs, *gc, *gl;
  double gz;
};

// the columns of right-hand side r: item_mode 0 = *c, 1 = ic[r], 2 = ic[0]
__device__ __forceinline__ MCols mcols(const MConst& c, const MConst* ic, int mode, int r) {
  MCols o;
  if (mode == 0) {
    o.gs = c.gs, o.gc = c.gc, o.gl = c.gl;
    o.gz = c.has_zm ? (c.total_volume * c.zm) * c.ls_o : 0.0;
  } else {
    const MConst* p = ic + (mode == 1 ? r : 0);
    o.gs = p->gs, o.gc = p->gc, o.gl = p->gl;
    o.gz = c.has_zm ? (p->total_volume * p->zm) * p->ls_o : 0.0;
  }
  return o;
}

// the column values of bins b0, b0 + 1 (0 past the end): 16-byte loads where
// both bins exist and the column is aligned
__device__ __forceinline__ void mload2(const double* p, long long b0, long long B, double& v0, double& v1) {
  v0 = v1 = 0.0;
  if (b0 + 1 < B && al16(p + b0)) {
    const double2 v = *reinterpret_cast<const double2*>(p + b0);
    v0 = v.x, v1 = v.y;
  } else {
    if (b0 < B) v0 = p[b0];
    if (b0 + 1 < B) v1 = p[b0 + 1];
  }
}

// one bin of the JVP: the same expression in every kernel, so a batched call
// is bitwise the single one
__device__ __forceinline__ double mjv(double gs, double gc, double gl, double ts, double tc, double tl) {
  return fma(gl, tl, fma(gc, tc, gs * ts));
}

// ------------------------------------------------------------------ forward
__global__ __launch_bounds__(MT) void matern_fwd(MModel m, const double* xs, const double* xc, const double* xl,
                                                 const double* xz, long long ls, double* a, long long as,
                                                 double* buf, long long bs, MConst* dcs) {
  const int r = blockIdx.y;
  const long long B = m.B, Bp = (B + 1) & ~1LL;
  const long long b = (long long)blockIdx.x * MT + threadIdx.x;
  const double s = exp(m.lm_s + m.ls_s * xs[r * ls]);
  const double cc = exp(m.lm_c + m.ls_c * xc[r * ls]);
  const double l = m.mu_l + m.sig_l * xl[r * ls];
  const double zm = m.has_zm ? exp(m.lm_o + m.ls_o * xz[r * ls]) : 0.0;
  double* gs = buf + r * bs;
  double* gc = gs + Bp;
  double* gl = gc + Bp;
  if (b < B) {
    double A = m.total_volume * zm, vs = 0.0, vc = 0.0, vl = 0.0;
    if (b > 0) {
      const double u = m.k2[b] / (cc * cc);
      const double lp = log1p(u);
      A = sqrt(m.total_volume) * s * exp(0.25 * l * lp);
      vs = m.ls_s * A;
      vc = -(0.5 * l * m.ls_c) * A * (u / (1.0 + u));
      vl = (0.25 * m.sig_l) * A * lp;
    }
    a[r * as + b] = A;
    gs[b] = vs, gc[b] = vc, gl[b] = vl;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    MConst c;
    c.gs = gs, c.gc = gc, c.gl = gl;
    c.l = l, c.zm = zm;
    c.ls_s = m.ls_s, c.sig_l = m.sig_l, c.ls_c = m.ls_c, c.ls_o = m.has_zm ? m.ls_o : 0.0;
    c.total_volume = m.total_volume;
    c.B = B;
    c.has_zm = m.has_zm;
    dcs[r] = c;
  }
}

// ---------------------------------------------------------------------- JVP
// any layout: da[r * ds + b * es], one right-hand side per blockIdx.y
__global__ __launch_bounds__(MT) void matern_jvp_gen(MConst c, const MConst* ic, int mode, const double* ts,
                                                     const double* tc, const double* tl, const double* tz,
                                                     long long ls, double* da, long long ds, long long es) {
  const int r = blockIdx.y;
  const long long B = c.B;
  const long long b0 = 2 * ((long long)blockIdx.x * MT + threadIdx.x);
  if (b0 >= B) return;
  const MCols k = mcols(c, ic, mode, r);
  const double vs = ts[r * ls], vc = tc[r * ls], vl = tl[r * ls], vz = tz ? tz[r * ls] : 0.0;
  double s0, s1, c0, c1, l0, l1;
  mload2(k.gs, b0, B, s0, s1);
  mload2(k.gc, b0, B, c0, c1);
  mload2(k.gl, b0, B, l0, l1);
  const double v0 = b0 == 0 ? k.gz * vz : mjv(s0, c0, l0, vs, vc, vl);
  const double v1 = mjv(s1, c1, l1, vs, vc, vl);
  double* row = da + r * ds;
  if (b0 + 1 < B && es == 1 && al16(row + b0)) {
    *reinterpret_cast<double2*>(row + b0) = make_double2(v0, v1);
  } else {
    row[b0 * es] = v0;
    if (b0 + 1 < B) row[(b0 + 1) * es] = v1;
  }
}

// bin-major interleaved, one constant set for all NR right-hand sides:
// da[b * NR + r]; a thread owns the 2 * NR contiguous values of two bins
template <int NR>
__global__ __launch_bounds__(MT) void matern_jvp_il(MConst c, const MConst* ic, int mode, const double* ts,
                                                    const double* tc, const double* tl, const double* tz,
                                                    long long ls, double* da) {
  const long long B = c.B;
  const long long b0 = 2 * ((long long)blockIdx.x * MT + threadIdx.x);
  if (b0 >= B) return;
  const MCols k = mcols(c, ic, mode, 0);
  double s0, s1, c0, c1, l0, l1;
  mload2(k.gs, b0, B, s0, s1);
  mload2(k.gc, b0, B, c0, c1);
  mload2(k.gl, b0, B, l0, l1);
  double v[2 * NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const double vs = ts[r * ls], vc = tc[r * ls], vl = tl[r * ls], vz = tz ? tz[r * ls] : 0.0;
    v[r] = b0 == 0 ? k.gz * vz : mjv(s0, c0, l0, vs, vc, vl);
    v[NR + r] = mjv(s1, c1, l1, vs, vc, vl);
  }
  double* o = da + b0 * NR;
  if (b0 + 1 < B && al16(o)) {
#pragma unroll
    for (int i = 0; i < NR; ++i) reinterpret_cast<double2*>(o)[i] = make_double2(v[2 * i], v[2 * i + 1]);
  } else {
#pragma unroll
    for (int i = 0; i < 2 * NR; ++i)
      if (i < NR || b0 + 1 < B) o[i] = v[i];
  }
}

// ---------------------------------------------------------------------- VJP
// sum over the workgroup of three values: wave shuffle tree, then the four
// wave sums in wave order (threads 0..2 return column tid's sum)
__device__ __forceinline__ double mreduce3(double p0, double p1, double p2, double (*red)[MT / 64]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    p0 += __shfl_down(p0, off, 64);
    p1 += __shfl_down(p1, off, 64);
    p2 += __shfl_down(p2, off, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[0][wave] = p0, red[1][wave] = p1, red[2][wave] = p2;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x < 3) s = ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
  __syncthreads();
  return s;
}

// per-workgroup partials ws[r * wsd + j * nb + blk] of column j over the
// workgroup's MTILE bins; a workgroup serves rper right-hand sides (all of
// them where they share one constant set: the columns are loaded once)
__global__ __launch_bounds__(MT) void matern_vjp_part(MConst c, const MConst* ic, int mode, const double* g,
                                                      long long gstr, int rper, int nrhs, double* ws, long long wsd,
                                                      int nb) {
  __shared__ double red[3][MT / 64];
  const long long B = c.B;
  const long long b0 = 2 * ((long long)blockIdx.x * MT + threadIdx.x);
  const int r0 = blockIdx.y * rper;
  double s0 = 0, s1 = 0, c0 = 0, c1 = 0, l0 = 0, l1 = 0;
  for (int i = 0; i < rper; ++i) {
    const int r = r0 + i;
    if (r >= nrhs) break;
    if (i == 0 || mode == 1) {
      const MCols k = mcols(c, ic, mode, r);
      mload2(k.gs, b0, B, s0, s1);
      mload2(k.gc, b0, B, c0, c1);
      mload2(k.gl, b0, B, l0, l1);
      if (b0 == 0) s0 = c0 = l0 = 0.0;  // the zero mode has its own column
    }
    double g0, g1;
    mload2(g + r * gstr, b0, B, g0, g1);
    const double s = mreduce3(fma(s1, g1, s0 * g0), fma(c1, g1, c0 * g0), fma(l1, g1, l0 * g0), red);
    if (threadIdx.x < 3) ws[r * wsd + (long long)threadIdx.x * nb + blockIdx.x] = s;
  }
}

struct MOut {
  double *o0, *o1, *o2, *o3;
  const double *d0, *d1, *d2, *d3;
};

// the fold: one workgroup per right-hand side sums each column's nb partials,
// thread t the partials t, t + MT, ... in order, then the workgroup sum; the
// order depends on nb = ceil(B / MTILE) alone
__global__ __launch_bounds__(MT) void matern_vjp_fold(MConst c, const MConst* ic, int mode, const double* g,
                                                      long long gstr, MOut o, long long ls, double shift,
                                                      const double* ws, long long wsd, int nb) {
  __shared__ double red[3][MT / 64];
  const int r = blockIdx.x;
  const double* w = ws + r * wsd;
  double p0 = 0.0, p1 = 0.0, p2 = 0.0;
  for (int blk = threadIdx.x; blk < nb; blk += MT) {
    p0 += w[blk];
    p1 += w[nb + blk];
    p2 += w[2 * nb + blk];
  }
  double s = mreduce3(p0, p1, p2, red);
  const int t = threadIdx.x;
  if (t > 3 || (t == 3 && !c.has_zm)) return;
  double* out = t == 0 ? o.o0 : t == 1 ? o.o1 : t == 2 ? o.o2 : o.o3;
  const double* d = t == 0 ? o.d0 : t == 1 ? o.d1 : t == 2 ? o.d2 : o.d3;
  if (t == 3) s = mcols(c, ic, mode, r).gz * g[r * gstr];
  out[r * ls] = d ? fma(shift, d[r * ls], s) : s;
}

static bool mconst_ok(const MConst* c, const MConst* ic, int mode) {
  if (!c || c->B < 2 || mode < 0 || mode > 2) return false;
  if (mode == 0) return c->gs && c->gc && c->gl;
  return ic != nullptr;
}

}  // namespace nft

using namespace nft;

extern "C" {

int64_t nft_matern_forward_buf(int64_t B) { return B < 2 ? 0 : 3 * ((B + 1) & ~(int64_t)1); }

size_t nft_matern_workspace(int64_t B) {
  if (B < 2) return 0;
  return (size_t)(3 * mblk(B, MTILE) + 1) / 2 * 2 * sizeof(double);
}

int nft_matern_forward_batched(const nft_matern_model* model, const double* x_scale, const double* x_cutoff,
                               const double* x_slope, const double* x_zm, int64_t lat_stride, int nrow, double* a,
                               int64_t a_stride, double* buf, int64_t buf_stride, nft_matern_const* item_consts,
                               hipStream_t s) {
  if (!model || model->B < 2 || nrow < 1 || !model->k2 || !x_scale || !x_cutoff || !x_slope ||
      (model->has_zm && !x_zm) || !a || !buf || !item_consts || lat_stride < 0 ||
      buf_stride < nft_matern_forward_buf(model->B) || a_stride < (nrow > 1 ? model->B : 0)) {
    set_last_error("nft_matern_forward_batched: invalid arguments");
    return NFT_ERR_ARG;
  }
  prof_mark(s, "matern_fwd");
  hipLaunchKernelGGL(matern_fwd, dim3(mblk(model->B, MT), (unsigned)nrow), dim3(MT), 0, s, *model, x_scale, x_cutoff,
                     x_slope, x_zm, (long long)lat_stride, a, (long long)a_stride, buf, (long long)buf_stride,
                     item_consts);
  NFT_HIP_CHECK(hipGetLastError());
  return NFT_OK;
}

int nft_matern_jvp_batched(const nft_matern_const* c, const nft_matern_const* item_consts, int item_mode,
                           const double* const* t, int64_t lat_stride, double* da, int64_t da_stride,
                           int64_t da_elem_stride, int nrhs, int dtype, hipStream_t s) {
  const int64_t es = da_elem_stride == 0 ? 1 : da_elem_stride;
  bool ok = mconst_ok(c, item_consts, item_mode) && nrhs >= 1 && dtype == 0 && t && t[0] && t[1] && t[2] && da &&
            lat_stride >= 0 && es >= 1 && da_stride >= 0;
  if (ok && c->has_zm && !t[3]) ok = false;
  if (ok && nrhs > 1) {
    // rows r * da_stride + b * es must not overlap: planar or bin-major
    const int64_t B = c->B;
    ok = da_stride >= (B - 1) * es + 1 || (da_stride >= 1 && es >= (nrhs - 1) * da_stride + 1);
  }
  if (!ok) {
    set_last_error("nft_matern_jvp_batched: invalid arguments (B >= 2, nrhs >= 1, fp64, non-null pointers, "
                   "da rows that do not overlap)");
    return NFT_ERR_ARG;
  }
  const MConst& k = *c;
  const long long ls = lat_stride;
  const double* tz = k.has_zm ? t[3] : nullptr;
  const unsigned nbx = (unsigned)mblk(k.B, MTILE);
  const bool il = item_mode != 1 && da_stride == 1 && es == nrhs && nrhs <= 8;
  prof_mark(s, "matern_jvp");
#define NFT_MJ(NR)                                                                                              \
  case NR:                                                                                                      \
    hipLaunchKernelGGL(matern_jvp_il<NR>, dim3(nbx), dim3(MT), 0, s, k, item_consts, item_mode, t[0], t[1], t[2], \
                       tz, ls, da);                                                                             \
    break;
  if (il && nrhs > 1) {
    switch (nrhs) {
      NFT_MJ(2) NFT_MJ(3) NFT_MJ(4) NFT_MJ(5) NFT_MJ(6) NFT_MJ(7) NFT_MJ(8)
    }
  } else {
    hipLaunchKernelGGL(matern_jvp_gen, dim3(nbx, (unsigned)nrhs), dim3(MT), 0, s, k, item_consts, item_mode, t[0],
                       t[1], t[2], tz, ls, da, (long long)da_stride, (long long)es);
  }
#undef NFT_MJ
  NFT_HIP_CHECK(hipGetLastError());
  return NFT_OK;
}

int nft_matern_vjp_batched(const nft_matern_const* c, const nft_matern_const* item_consts, int item_mode,
                           const double* g, int64_t g_stride, double* const* out, const double* const* d,
                           int64_t lat_stride, double shift, double* ws, int nrhs, hipStream_t s) {
  bool ok = mconst_ok(c, item_consts, item_mode) && nrhs >= 1 && g && out && out[0] && out[1] && out[2] && ws &&
            lat_stride >= 0 && g_stride >= 0;
  if (ok && c->has_zm && !out[3]) ok = false;
  const bool use_d = ok && d != nullptr && shift != 0.0;
  if (use_d && (!d[0] || !d[1] || !d[2] || (c->has_zm && !d[3]))) ok = false;
  // rows of g and of the outputs must not overlap
  if (ok && nrhs > 1 && (g_stride < c->B || lat_stride < 1)) ok = false;
  if (!ok) {
    set_last_error("nft_matern_vjp_batched: invalid arguments (B >= 2, nrhs >= 1, non-null pointers, "
                   "g_stride >= B and lat_stride >= 1 for nrhs > 1)");
    return NFT_ERR_ARG;
  }
  const MConst& k = *c;
  const int nb = mblk(k.B, MTILE);
  const long long wsd = (long long)(nft_matern_workspace(k.B) / sizeof(double));
  const int rper = item_mode == 1 ? 1 : nrhs;
  prof_mark(s, "matern_vjp_part");
  hipLaunchKernelGGL(matern_vjp_part, dim3((unsigned)nb, (unsigned)((nrhs + rper - 1) / rper)), dim3(MT), 0, s, k,
                     item_consts, item_mode, g, (long long)g_stride, rper, nrhs, ws, wsd, nb);
  MOut o;
  o.o0 = out[0], o.o1 = out[1], o.o2 = out[2], o.o3 = k.has_zm ? out[3] : nullptr;
  o.d0 = use_d ? d[0] : nullptr, o.d1 = use_d ? d[1] : nullptr, o.d2 = use_d ? d[2] : nullptr;
  o.d3 = use_d && k.has_zm ? d[3] : nullptr;
  prof_mark(s, "matern_vjp_fold");
  hipLaunchKernelGGL(matern_vjp_fold, dim3((unsigned)nrhs), dim3(MT), 0, s, k, item_consts, item_mode, g,
                     (long long)g_stride, o, (long long)lat_stride, shift, ws, wsd, nb);
  NFT_HIP_CHECK(hipGetLastError());
  return NFT_OK;
}

}  // extern "C"
