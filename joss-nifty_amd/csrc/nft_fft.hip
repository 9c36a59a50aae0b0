// Batched multi-dimensional FFT / genuine Hartley transforms for gfx950.
//
// Replaces the numeric seam of the reference, src/ducc_dispatch.py:
//   fftn / ifftn  (:38-43, :66-72)  -> nft_fft_c2c
//   hartley       (:46-50, :75-78)  -> nft_hartley   (both conventions,
//                                      src/config.py:3-40)
//
// Multi-axis real Hartley over axes A = {a_0 < ... < a_{m-1}}:
//   pass 1      R2C along h = a_{m-1}: real -> complex half spectrum
//               (two real lines per complex FFT)
//   passes 2..  C2C along a_{m-2} ... a_1 (in place on the half spectrum)
//   last pass   C2C along a_0 + UNPACK: H(k) = Re F(k) + s Im F(k) and
//               H(-k) = Re F(k) - s Im F(k) written from the same line.
// Every pass is one HBM read + one HBM write of the field (a d-dim transform
// costs d passes); the half spectrum is ~N complex/2 = N reals.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "fast_dispatch.hpp"
#include "fft_passes.hpp"
#include <type_traits>

#include "nft_api_internal.hpp"

namespace nft {

// ------------------------------------------------------------ error handling
static thread_local char g_last_error[1024] = "";
void set_last_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_last_error, sizeof(g_last_error), fmt, ap);
  va_end(ap);
}
const char* last_error() { return g_last_error; }

// ------------------------------------------------------------ twiddle tables
struct TwKey {
  int dev, n, dtype;
  bool operator<(const TwKey& o) const {
    if (dev != o.dev) return dev < o.dev;
    if (n != o.n) return n < o.n;
    return dtype < o.dtype;
  }
};
static std::map<TwKey, void*> g_tw;
static std::mutex g_tw_mu;

// exp(-2 pi i k / n) with exact symmetries (octant reduction in long double)
static void twiddle_host(int n, std::vector<long double>& re, std::vector<long double>& im) {
  // W^k = exp(-2 pi i k/n), k < n.  Built from the first quadrant by exact
  // rotations, W^(k + n/4) = -i W^k, so the device may keep only the quarter
  // table (fft_fast.hpp: tw_at) and reproduce every entry bit for bit; inside
  // the quadrant the octant symmetry keeps the evaluated angle <= pi/4.
  re.resize(n);
  im.resize(n);
  const long double pi = 3.141592653589793238462643383279502884L;
  if (n % 4 != 0) {  // lengths of the generic engine: direct evaluation
    for (int k = 0; k < n; ++k) {
      const long double a = 2.0L * pi * (long double)k / (long double)n;
      long double c = cosl(a), s = sinl(a);
      if (2LL * k == n) {
        c = -1;
        s = 0;
      }
      if (k == 0) {
        c = 1;
        s = 0;
      }
      re[k] = c;
      im[k] = -s;
    }
    return;
  }
  const int q4 = n / 4;
  std::vector<long double> c0(q4), s0(q4);
  for (int r = 0; r < q4; ++r) {
    if (8LL * r <= n) {
      const long double a = 2.0L * pi * (long double)r / (long double)n;
      c0[r] = cosl(a);
      s0[r] = sinl(a);
    } else {  // pi/2 - a' with a' = 2 pi (n/4 - r)/n <= pi/4
      const long double a = 2.0L * pi * (long double)(q4 - r) / (long double)n;
      c0[r] = sinl(a);
      s0[r] = cosl(a);
    }
  }
  for (int k = 0; k < n; ++k) {
    const int q = k / q4, r = k - q * q4;
    long double wr = c0[r], wi = -s0[r];
    for (int t = 0; t < q; ++t) {  // multiply by -i
      const long double tmp = wr;
      wr = wi;
      wi = -tmp;
    }
    re[k] = wr;
    im[k] = wi;
  }
}

int get_twiddles(int n, int dtype, const void** out) {
  int dev = 0;
  NFT_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_tw_mu);
  TwKey key{dev, n, dtype};
  auto it = g_tw.find(key);
  if (it != g_tw.end()) {
    *out = it->second;
    return NFT_OK;
  }
  std::vector<long double> re, im;
  twiddle_host(n, re, im);
  void* d = nullptr;
  if (dtype == 0) {
    std::vector<double2> h(n);
    for (int k = 0; k < n; ++k) h[k] = double2{(double)re[k], (double)im[k]};
    NFT_HIP_CHECK(hipMalloc(&d, sizeof(double2) * n));
    NFT_HIP_CHECK(hipMemcpy(d, h.data(), sizeof(double2) * n, hipMemcpyHostToDevice));
  } else {
    std::vector<float2> h(n);
    for (int k = 0; k < n; ++k) h[k] = float2{(float)re[k], (float)im[k]};
    NFT_HIP_CHECK(hipMalloc(&d, sizeof(float2) * n));
    NFT_HIP_CHECK(hipMemcpy(d, h.data(), sizeof(float2) * n, hipMemcpyHostToDevice));
  }
  g_tw[key] = d;
  *out = d;
  return NFT_OK;
}

void free_twiddles() {
  std::lock_guard<std::mutex> lk(g_tw_mu);
  for (auto& kv : g_tw) (void)hipFree(kv.second);
  g_tw.clear();
}

// ------------------------------------------------------------ plans
FftPlanDev make_plan(int n) {
  FftPlanDev p;
  memset(&p, 0, sizeof(p));
  p.n = n;
  int m = n, s = 0;
  const int order[] = {8, 4, 2, 3, 5, 7};
  for (int r : order) {
    while (m % r == 0 && s < FFT_MAXSTAGES) {
      p.radix[s++] = r;
      m /= r;
    }
  }
  if (m != 1) s = 0;  // large prime factor: direct DFT
  p.nstages = s;
  return p;
}

// VPT/NT instantiations
constexpr int VPT = 16;

// does a tile of L lines satisfy the per-stage register capacity?
static bool plan_fits(const FftPlanDev& p, int L, int NT) {
  long long tot = (long long)L * p.n;
  if (p.nstages == 0) return tot <= (long long)NT * VPT;
  for (int s = 0; s < p.nstages; ++s) {
    int R = p.radix[s];
    long long nbf = tot / R;
    if (nbf > (long long)NT * (VPT / R)) return false;
  }
  return true;
}

static size_t lds_budget() { return (size_t)65536; }

// choose NT, L, pitch for a pass of length n, element size es, tiling mode
struct LaunchCfg {
  int NT, L, pitch;
  size_t lds;
};

static int choose_cfg(const FftPlanDev& p, size_t es, bool rows, long long nlines, LaunchCfg& c) {
  const int nts[] = {256, 512, 1024};
  for (int NT : nts) {
    // rows: pitch = n; strided: pitch = n + 1 (breaks power-of-two bank aliasing)
    int pitch = rows ? p.n : p.n + 1;
    int Lmax = 1;
    while (plan_fits(p, Lmax * 2, NT) && (size_t)(Lmax * 2) * pitch * es <= lds_budget() &&
           Lmax * 2 <= 1024)
      Lmax *= 2;
    if (!plan_fits(p, 1, NT)) continue;
    size_t need = (size_t)pitch * es;
    if (need > 163840) return NFT_ERR_UNSUPPORTED;
    int L = Lmax;
    // do not make tiles much larger than the number of lines available
    while (L > 1 && L / 2 >= nlines) L /= 2;
    c.NT = NT;
    c.L = L;
    c.pitch = pitch;
    c.lds = (size_t)L * pitch * es + (size_t)L * sizeof(UnpackLine) + 16;
    if (c.lds > 163840) return NFT_ERR_UNSUPPORTED;
    return NFT_OK;
  }
  return NFT_ERR_UNSUPPORTED;
}

// ------------------------------------------------------------ kernels
enum PassKind { PK_C2C = 0, PK_R2C = 1, PK_H1D = 2, PK_UNPACK = 3 };

template <typename T, int NT, int KIND>
__global__ __launch_bounds__(NT) void pass_kernel(PassArgs<T> a) {
  extern __shared__ __align__(16) unsigned char smem[];
  using C = cplx_t<T>;
  C* lds = (C*)smem;
  const long long tile = blockIdx.x;
  if constexpr (KIND == PK_C2C || KIND == PK_UNPACK) load_c<T, NT>(a, tile, lds);
  else load_rp<T, NT>(a, tile, lds);
  __syncthreads();
  lds_fft<T, VPT, NT>(lds, a.pitch, a.L, a.plan, (const C*)a.tw, threadIdx.x);
  if constexpr (KIND == PK_C2C) store_c<T, NT>(a, tile, lds);
  else if constexpr (KIND == PK_R2C) store_r2c<T, NT>(a, tile, lds);
  else if constexpr (KIND == PK_H1D) store_h1d<T, NT>(a, tile, lds);
  else {
    UnpackLine* lines = (UnpackLine*)(smem + (size_t)a.L * a.pitch * sizeof(C));
    store_unpack<T, NT>(a, tile, lds, lines);
  }
}

template <typename T, int KIND>
static int launch_kind(const PassArgs<T>& a, const LaunchCfg& c, long long ntiles, hipStream_t s) {
  if (ntiles <= 0) return NFT_OK;
  if (ntiles > 0x7fffffffLL) {
    set_last_error("too many tiles (%lld)", ntiles);
    return NFT_ERR_UNSUPPORTED;
  }
  dim3 grid((unsigned)ntiles), block(c.NT);
  switch (c.NT) {
    case 256:
      hipLaunchKernelGGL((pass_kernel<T, 256, KIND>), grid, block, c.lds, s, a);
      break;
    case 512:
      hipLaunchKernelGGL((pass_kernel<T, 512, KIND>), grid, block, c.lds, s, a);
      break;
    case 1024:
      hipLaunchKernelGGL((pass_kernel<T, 1024, KIND>), grid, block, c.lds, s, a);
      break;
    default: return NFT_ERR_UNSUPPORTED;
  }
  NFT_HIP_CHECK(hipGetLastError());
  return NFT_OK;
}

template <typename T>
static int launch_pass(int kind, PassArgs<T>& a, hipStream_t s) {
  size_t es = sizeof(cplx_t<T>);
  LaunchCfg c;
  long long nl = a.rows ? a.O : a.I;
  int st = choose_cfg(a.plan, es, a.rows != 0, nl, c);
  if (st != NFT_OK) {
    set_last_error("unsupported FFT length %d", a.plan.n);
    return st;
  }
  a.L = c.L;
  a.pitch = c.pitch;
  const void* tw = nullptr;
  st = get_twiddles(a.plan.n, sizeof(T) == 8 ? 0 : 1, &tw);
  if (st != NFT_OK) return st;
  a.tw = tw;
  long long ntiles = a.rows ? (a.O + a.L - 1) / a.L : a.O * ((a.I + a.L - 1) / a.L);
  switch (kind) {
    case PK_C2C: return launch_kind<T, PK_C2C>(a, c, ntiles, s);
    case PK_R2C: return launch_kind<T, PK_R2C>(a, c, ntiles, s);
    case PK_H1D: return launch_kind<T, PK_H1D>(a, c, ntiles, s);
    case PK_UNPACK: return launch_kind<T, PK_UNPACK>(a, c, ntiles, s);
  }
  return NFT_ERR_ARG;
}

// ------------------------------------------------------------ geometry helpers
struct Geo {
  int nd;
  long long shape[MAXD];
};

static long long prod(const long long* s, int a, int b) {
  long long p = 1;
  for (int k = a; k < b; ++k) p *= s[k];
  return p;
}

static int parse_axes(int ndim, const int64_t* shape, int naxes, const int* axes, Geo& g,
                      std::vector<int>& ax) {
  if (ndim < 1 || ndim > MAXD) {
    set_last_error("ndim %d out of range [1, %d]", ndim, MAXD);
    return NFT_ERR_ARG;
  }
  g.nd = ndim;
  for (int k = 0; k < ndim; ++k) {
    if (shape[k] < 1) {
      set_last_error("empty dimension");
      return NFT_ERR_ARG;
    }
    g.shape[k] = shape[k];
  }
  std::vector<int> seen(ndim, 0);
  for (int k = 0; k < naxes; ++k) {
    int a = axes[k];
    if (a < 0) a += ndim;
    if (a < 0 || a >= ndim) {
      set_last_error("axis %d out of range", axes[k]);
      return NFT_ERR_ARG;
    }
    if (!seen[a]) ax.push_back(a);
    seen[a] = 1;
  }
  std::sort(ax.begin(), ax.end());
  return NFT_OK;
}

// complex half-spectrum buffer shape for a Hartley over `ax` (half dim = ax.back())
static void half_shape(const Geo& g, int h, long long* cs) {
  for (int k = 0; k < g.nd; ++k) cs[k] = g.shape[k];
  cs[h] = g.shape[h] / 2 + 1;
  if (h == g.nd - 1) cs[h] = (cs[h] + 7) / 8 * 8;
}

template <typename T>
static void fill_line_geom(PassArgs<T>& a, const long long* in_shape, const long long* out_shape,
                           int nd, int axis) {
  // C-contiguous strides
  long long Iin = prod(in_shape, axis + 1, nd), Iout = prod(out_shape, axis + 1, nd);
  a.in_sn = Iin;
  a.in_si = 1;
  a.in_so = Iin * in_shape[axis];
  a.out_sn = Iout;
  a.out_si = 1;
  a.out_so = Iout * out_shape[axis];
  a.O = prod(in_shape, 0, axis);
  a.I = Iin;
  a.rows = (axis == nd - 1);
}

template <typename T>
static int hartley_impl(const void* in, void* out, const Geo& g, const std::vector<int>& ax,
                        int sigma, double scale, void* ws, size_t ws_bytes, hipStream_t s) {
  const int m = (int)ax.size();
  if (m == 0) {
    long long N = prod(g.shape, 0, g.nd);
    if (in != out) NFT_HIP_CHECK(hipMemcpyAsync(out, in, N * sizeof(T), hipMemcpyDeviceToDevice, s));
    if (scale != 1.0) return scale_real(out, N, sizeof(T) == 8 ? 0 : 1, scale, s);
    return NFT_OK;
  }
  if (m == 1) {
    int axis = ax[0];
    PassArgs<T> a;
    memset(&a, 0, sizeof(a));
    a.plan = make_plan((int)g.shape[axis]);
    a.in = in;
    a.out = out;
    fill_line_geom(a, g.shape, g.shape, g.nd, axis);
    a.sigma = sigma;
    a.scale = (T)scale;
    if (a.rows) {
      a.Ireal = a.O;
      a.O = (a.O + 1) / 2;
    } else {
      a.Ireal = a.I;
      a.I = (a.I + 1) / 2;
    }
    if (in == out) {
      // H1D reads two lines fully into LDS before writing them back: safe in place
    }
    return launch_pass<T>(PK_H1D, a, s);
  }
  const int h = ax[m - 1];
  long long cs[MAXD];
  half_shape(g, h, cs);
  size_t need = (size_t)prod(cs, 0, g.nd) * sizeof(cplx_t<T>);
  if (ws == nullptr || ws_bytes < need) {
    set_last_error("hartley workspace too small (%zu < %zu)", ws_bytes, need);
    return NFT_ERR_ARG;
  }
  // pass 1: R2C along h
  {
    PassArgs<T> a;
    memset(&a, 0, sizeof(a));
    a.plan = make_plan((int)g.shape[h]);
    a.in = in;
    a.out = ws;
    fill_line_geom(a, g.shape, cs, g.nd, h);
    a.scale = (T)1;
    if (a.rows) {
      a.Ireal = a.O;
      a.O = (a.O + 1) / 2;
    } else {
      a.Ireal = a.I;
      a.I = (a.I + 1) / 2;
    }
    int st = launch_pass<T>(PK_R2C, a, s);
    if (st != NFT_OK) return st;
  }
  // middle passes: C2C in place
  for (int k = m - 2; k >= 1; --k) {
    int axis = ax[k];
    PassArgs<T> a;
    memset(&a, 0, sizeof(a));
    a.plan = make_plan((int)g.shape[axis]);
    a.in = ws;
    a.out = ws;
    fill_line_geom(a, cs, cs, g.nd, axis);
    a.scale = (T)1;
    int st = launch_pass<T>(PK_C2C, a, s);
    if (st != NFT_OK) return st;
  }
  // last pass: C2C along ax[0] + unpack to real
  {
    int axis = ax[0];
    PassArgs<T> a;
    memset(&a, 0, sizeof(a));
    a.plan = make_plan((int)g.shape[axis]);
    a.in = ws;
    a.out = out;
    fill_line_geom(a, cs, g.shape, g.nd, axis);
    // input line geometry from cs, output via LineDesc
    a.sigma = sigma;
    a.scale = (T)scale;
    LineDesc& d = a.desc;
    memset(&d, 0, sizeof(d));
    d.nout = axis;
    d.nin = g.nd - axis - 1;
    d.half = -1;
    long long rs[MAXD];
    rs[g.nd - 1] = 1;
    for (int k = g.nd - 2; k >= 0; --k) rs[k] = rs[k + 1] * g.shape[k + 1];
    int j = 0;
    for (int k = 0; k < g.nd; ++k) {
      if (k == axis) continue;
      d.ext[j] = (int)cs[k];
      d.rstride[j] = rs[k];
      d.nreal[j] = (int)g.shape[k];
      d.neg[j] = std::find(ax.begin(), ax.end(), k) != ax.end();
      if (k == h) d.half = j;
      ++j;
    }
    a.out_sn = rs[axis];
    return launch_pass<T>(PK_UNPACK, a, s);
  }
}

// ------------------------------------------------------------ engine v2 path
constexpr int NFT_FALLBACK = 1;  // geometry not covered by engine v2

static LineDesc make_desc(const Geo& g, const long long* cs, const std::vector<int>& ax, int axis, int h) {
  LineDesc d;
  memset(&d, 0, sizeof(d));
  d.nout = axis;
  d.nin = g.nd - axis - 1;
  d.half = -1;
  long long rs[MAXD];
  rs[g.nd - 1] = 1;
  for (int k = g.nd - 2; k >= 0; --k) rs[k] = rs[k + 1] * g.shape[k + 1];
  int j = 0;
  for (int k = 0; k < g.nd; ++k) {
    if (k == axis) continue;
    d.ext[j] = (int)cs[k];
    d.rstride[j] = rs[k];
    d.nreal[j] = (int)g.shape[k];
    d.neg[j] = std::find(ax.begin(), ax.end(), k) != ax.end();
    if (k == h) d.half = j;
    ++j;
  }
  return d;
}

// geometry covered by hartley_v2's multi-axis path (its first launch is the
// R2C row pass along the last axis)
static bool v2_multi_ok(const Geo& g, const std::vector<int>& ax) {
  using namespace fast;
  const int m = (int)ax.size();
  if (m < 2) return false;
  const int h = ax[m - 1];
  if (h != g.nd - 1 || !rows_supported((int)g.shape[h])) return false;
  for (int k = 1; k < m - 1; ++k)
    if (!strided_supported((int)g.shape[ax[k]])) return false;
  const int N0 = (int)g.shape[ax[0]];
  return strided_supported(N0) || fourstep_supported(N0);
}

// r2c_done: the R2C row pass has already written the half spectra to ws
template <typename T>
static int hartley_v2(const void* in, void* out, const Geo& g, const std::vector<int>& ax, int sigma,
                      double scale, void* ws, size_t ws_bytes, hipStream_t s,
                      const fast::FuseArgs* fz = nullptr, bool r2c_done = false) {
  using namespace fast;
  const int m = (int)ax.size();
  const int last = g.nd - 1;
  if (m == 0) return NFT_FALLBACK;
  if (m == 1) {
    const int N = (int)g.shape[ax[0]];
    if (ax[0] != last || !rows_supported(N)) return NFT_FALLBACK;
    FastArgs<T> a;
    memset(&a, 0, sizeof(a));
    a.in = in;
    a.out = out;
    a.g.O = prod(g.shape, 0, last);
    a.g.M = a.g.I = 1;
    a.g.in_so = a.g.out_so = N;
    a.g.in_sn = a.g.out_sn = 1;
    a.Ireal = a.g.O;
    a.sigma = sigma;
    a.scale = (T)scale;
    if (fz) a.f = *fz;
    return launch<T>(K_H1D, true, N, a, s);
  }
  const int h = ax[m - 1];
  if (h != last || !rows_supported((int)g.shape[h])) return NFT_FALLBACK;
  for (int k = 1; k < m - 1; ++k)
    if (!strided_supported((int)g.shape[ax[k]])) return NFT_FALLBACK;
  const int N0 = (int)g.shape[ax[0]];
  if (!strided_supported(N0) && !fourstep_supported(N0)) return NFT_FALLBACK;
  long long cs[MAXD];
  half_shape(g, h, cs);
  size_t need = (size_t)prod(cs, 0, g.nd) * sizeof(cplx_t<T>);
  if (ws == nullptr || ws_bytes < need) {
    set_last_error("hartley workspace too small (%zu < %zu)", ws_bytes, need);
    return NFT_ERR_ARG;
  }
  int st;
  if (!r2c_done) {  // R2C rows along the last axis
    const int N = (int)g.shape[h];
    FastArgs<T> a;
    memset(&a, 0, sizeof(a));
    a.in = in;
    a.out = ws;
    a.g.O = prod(g.shape, 0, last);
    a.g.M = a.g.I = 1;
    a.g.in_so = N;
    a.g.in_sn = 1;
    a.g.out_so = cs[last];
    a.g.out_sn = 1;
    a.Ireal = a.g.O;
    a.scale = (T)1;
    if (fz) {
      a.f = *fz;
      a.f.epi = 0;
      a.f.cg = 0;
      a.f.quad = 0;
    }
    if ((st = launch<T>(K_R2C, true, N, a, s)) != NFT_OK) return st;
  }
  for (int k = m - 2; k >= 1; --k) {  // middle axes, strided C2C in place
    const int axis = ax[k];
    const int N = (int)g.shape[axis];
    const long long I = prod(cs, axis + 1, g.nd);
    FastArgs<T> a;
    memset(&a, 0, sizeof(a));
    a.in = ws;
    a.out = ws;
    a.g.O = prod(cs, 0, axis);
    a.g.M = 1;
    a.g.I = I;
    a.g.in_so = a.g.out_so = I * N;
    a.g.in_si = a.g.out_si = 1;
    a.g.in_sn = a.g.out_sn = I;
    a.scale = (T)1;
    if ((st = launch<T>(K_C2C, false, N, a, s)) != NFT_OK) return st;
  }
  {  // last pass along ax[0]: C2C + unpack to real (four-step for long axes)
    const int axis = ax[0];
    const int N = N0;
    const long long I = prod(cs, axis + 1, g.nd);
    const long long O = prod(cs, 0, axis);
    const long long rrs = prod(g.shape, axis + 1, g.nd);
    LineDesc desc = make_desc(g, cs, ax, axis, h);
    if (strided_supported(N)) {
      FastArgs<T> a;
      memset(&a, 0, sizeof(a));
      a.in = ws;
      a.out = out;
      a.g.O = O;
      a.g.M = 1;
      a.g.I = I;
      a.g.in_so = I * N;
      a.g.in_si = 1;
      a.g.in_sn = I;
      a.km = 0;
      a.kx = 1;
      a.Nfull = N;
      a.rs = rrs;
      a.sigma = sigma;
      a.scale = (T)scale;
      a.desc = desc;
      if (fz) {
        a.f = *fz;
        a.f.pro = 0;
        a.f.fnrhs = 0;  // the fold rides in the R2C pass
      }
      return launch<T>(K_UNPACK, false, N, a, s);
    }
    int N1, N2;
    fourstep_split(N, N1, N2);
    const void* twN = nullptr;
    if ((st = get_twiddles(N, sizeof(T) == 8 ? 0 : 1, &twN)) != NFT_OK) return st;
    {  // A: length-N1 FFTs over rows n2 + N2*j, post-twiddle W_N^(n2*k1), in place
      FastArgs<T> a;
      memset(&a, 0, sizeof(a));
      a.in = ws;
      a.out = ws;
      a.g.O = O;
      a.g.M = N2;
      a.g.I = I;
      a.g.in_so = a.g.out_so = I * N;
      a.g.in_sm = a.g.out_sm = I;
      a.g.in_si = a.g.out_si = 1;
      a.g.in_sn = a.g.out_sn = I * N2;
      a.tw2 = twN;
      a.Nfull = N;
      a.scale = (T)1;
      if ((st = launch<T>(K_C2C, false, N1, a, s)) != NFT_OK) return st;
    }
    {  // B: length-N2 FFTs over rows N2*k1 + n2; element k2 -> k = k1 + N1*k2; unpack
      FastArgs<T> a;
      memset(&a, 0, sizeof(a));
      a.in = ws;
      a.out = out;
      a.g.O = O;
      a.g.M = N1;
      a.g.I = I;
      a.g.in_so = I * N;
      a.g.in_sm = I * N2;
      a.g.in_si = 1;
      a.g.in_sn = I;
      a.km = 1;
      a.kx = N1;
      a.Nfull = N;
      a.rs = rrs;
      a.sigma = sigma;
      a.scale = (T)scale;
      a.desc = desc;
      if (fz) {
        a.f = *fz;
        a.f.pro = 0;
        a.f.fnrhs = 0;  // the fold rides in the R2C pass
      }
      return launch<T>(K_UNPACK, false, N2, a, s);
    }
  }
}

static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// unfused fallback of nft_hartley_fused: prologue / epilogue as elementwise passes
template <typename T>
__global__ void fuse_pro_kernel(fast::FuseArgs f, T* __restrict__ dst, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    dst[i] = fast::fuse_pro<T>(f, i);
}

template <typename T>
__global__ void fuse_epi_kernel(fast::FuseArgs f, const T* __restrict__ h, T* __restrict__ out, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    fast::fuse_store<T>(f, out, i, h[i]);
}

// Prologue of a batch of items sharing pa / pb / pidx (the CF Jacobian's
// A_full, xi0 and bin index), as its own streaming pass: thread j reads the
// shared operands of element j once and forms u[b][j] for every item b.
// Inside the R2C row pass the same prologue is latency-bound (dependent bin
// gathers at 4 workgroups per CU, shared operands re-read per item: 196 us
// for 4 items at 2048^2 vs 67 us for the plain pass); split, the plain pass
// runs persistent and prefetching.  Same arithmetic per element as
// fast::fuse_pro (bitwise).
template <typename T>
__global__ __launch_bounds__(256) void pro_batch_kernel(fast::FuseArgs f, T* __restrict__ u, long long P,
                                                        int nb) {
  // restrict-qualified: the loads of the next element may be issued before
  // the stores of this one
  const T* __restrict__ px = (const T*)f.px;
  const T* __restrict__ pa = (const T*)f.pa;
  const T* __restrict__ pb = (const T*)f.pb;
  const T* __restrict__ pc = (const T*)f.pc;
  using V2 = typename std::conditional<sizeof(T) == 8, double2, float2>::type;
  // interleaved dA (ce == nb, sc == 1): each pixel's gather is one contiguous
  // run; read it with 2-wide vector loads (half the divergent load
  // instructions: the gather is bound by distinct lines per instruction)
  const bool vec = pb && f.ce == nb && f.sc == 1 && (nb & 1) == 0;
  for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < P; j += (long long)gridDim.x * 256) {
    const T a = pa ? pa[j] : (T)1;
    const T bj = pb ? pb[j] : (T)0;
    const long long ix = pb ? pro_cidx(f, j) : 0;  // element index (pindex or folded cell) x ce
    if (vec) {
      const V2* q = (const V2*)(pc + ix);
#pragma unroll 2
      for (int bp = 0; bp < nb / 2; ++bp) {
        const V2 c2 = q[bp];
        T v0 = px[(2 * bp) * f.sx + j], v1 = px[(2 * bp + 1) * f.sx + j];
        if (pa) {
          v0 *= a;
          v1 *= a;
        }
        v0 += bj * c2.x;
        v1 += bj * c2.y;
        u[(2 * bp) * P + j] = v0;
        u[(2 * bp + 1) * P + j] = v1;
      }
      continue;
    }
#pragma unroll 4
    for (int b = 0; b < nb; ++b) {
      T v = px[b * f.sx + j];
      if (pa) v *= a;
      if (pb) v += bj * pc[b * f.sc + ix];
      u[b * P + j] = v;
    }
  }
}

// Folded prologue of a batch (nft_hartley_fuse.pro_folded): one thread per
// fundamental cell c reads the cell's bin (coalesced), gathers the dA run of
// that bin for all items once, and forms u at every distinct mirror image
// of c (2^d pixels, fewer on self-mirror axes) -- each image's x, A, xi0 and
// u accesses are contiguous across the wave (forward or reversed).  Same
// arithmetic per element as pro_batch_kernel (bitwise).
// D (the number of transform axes) is a template parameter so that the cell
// coordinates and the per-item values stay in registers (a runtime D put
// them in scratch).
// images per load group of the folded prologue (1 / 4 measured 136 / 203 us
// against 132 for 2 at 4 x 2048^2)
constexpr int PRO_G = 2;
template <typename T, int D, int NBM, bool PI>
__global__ __launch_bounds__(256) void pro_fold_kernel(fast::FuseArgs f, T* __restrict__ u, long long P, int nb,
                                                       long long ncell) {
  // PI: A and xi0 per item (rows f.sa / f.sb apart: the batched geoVI
  // refinement's per-sample Jacobians), else shared by the items
  // NBM: register capacity for the items (nb <= NBM; nb > 8 runs the item
  // loop of the last branch with NBM = 8)
  const T* __restrict__ px = (const T*)f.px;
  const T* __restrict__ pa = (const T*)f.pa;
  const T* __restrict__ pb = (const T*)f.pb;
  const T* __restrict__ pc = (const T*)f.pc;
  using V2 = typename std::conditional<sizeof(T) == 8, double2, float2>::type;
  const bool vec = f.ce == nb && f.sc == 1 && (nb & 1) == 0 && nb <= NBM;
  // the CG direction update carried here (f.dr): d = max(0, gamma/gprev) d + r
  // per item, written back to px, d.d accumulated per item (nb <= 8)
  const bool dirc = f.dr != nullptr;
  T* pd = const_cast<T*>(px);
  const T* __restrict__ pr = (const T*)f.dr;
  T bt[NBM];
  bool live[NBM];
  double dd[NBM];
#pragma unroll
  for (int b = 0; b < NBM; ++b) {
    dd[b] = 0.0;
    bt[b] = (T)0;
    live[b] = false;
    if (dirc && b < nb) {
      const double* scb = f.dsc + b * NFT_CG_NSCALARS;
      live[b] = scb[NFT_CG_DONE] == 0.0;
      double beta = scb[NFT_CG_GAMMA] / scb[NFT_CG_GPREV];
      if (!(beta > 0.0)) beta = 0.0;
      bt[b] = (T)beta;
    }
  }
  unsigned nn[D];
#pragma unroll
  for (int a = 0; a < D; ++a) nn[a] = (unsigned)f.fn[a];
  // threads walk the cell grid with its last axis padded to hp (a multiple
  // of 64): each wave covers one aligned run of a cell row, so its direct
  // images are whole cache lines and its mirrored ones share their one
  // unaligned line with the neighbouring wave
  const unsigned hl = nn[D - 1] / 2 + 1, hp = (hl + 63) & ~63u;
  // images in groups of G: every load of a group (x, r, A, xi0 of all its
  // images and items) is issued before its first store -- d is stored back
  // into the array x is read from, so a load cannot pass an earlier store
  // and per-image load / store pairs would serialise one memory round trip
  // per image and item
  constexpr int NIMG = 1 << D;
  constexpr int G0 = PRO_G;
  constexpr int G = G0 < NIMG ? G0 : NIMG;
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < ncell; c += (long long)gridDim.x * 256) {
    unsigned cc[D], rest = (unsigned)c;
    {
      const unsigned q = rest / hp;
      cc[D - 1] = rest - q * hp;
      rest = q;
    }
    if (cc[D - 1] >= hl) continue;
#pragma unroll
    for (int a = D - 2; a >= 0; --a) {
      const unsigned h = nn[a] / 2 + 1;
      const unsigned q = rest / h;
      cc[a] = rest - q * h;
      rest = q;
    }
    unsigned cell = 0;
#pragma unroll
    for (int a = 0; a < D; ++a) cell = cell * (nn[a] / 2 + 1) + cc[a];
    const long long ix = (long long)f.pidx[cell] * f.ce;
    T cv[NBM];
#pragma unroll
    for (int b = 0; b < NBM; ++b) cv[b] = (T)0;
    if (vec) {
      const V2* q = (const V2*)(pc + ix);
#pragma unroll
      for (int bp = 0; bp < NBM / 2; ++bp)
        if (2 * bp < nb) {
          const V2 c2 = q[bp];
          cv[2 * bp] = c2.x;
          cv[2 * bp + 1] = c2.y;
        }
    } else if (nb <= NBM) {
#pragma unroll
      for (int b = 0; b < NBM; ++b)
        if (b < nb) cv[b] = pc[b * f.sc + ix];
    }
    // images: bit a of m flips axis a (skipped when that axis is self-mirror)
    auto image = [&](int m, unsigned& j) {
      j = 0;
      bool dup = false;
#pragma unroll
      for (int a = 0; a < D; ++a) {
        unsigned k = cc[a];
        if ((m >> a) & 1) {
          const unsigned km = k == 0 ? 0 : nn[a] - k;
          if (km == k) dup = true;
          k = km;
        }
        j = j * nn[a] + k;
      }
      return !dup;
    };
    if (nb > NBM) {  // large batches (no carried direction): items in a loop
#pragma unroll
      for (int m = 0; m < NIMG; ++m) {
        unsigned j;
        if (!image(m, j)) continue;
        const T a = pa ? pa[j] : (T)1;
        const T bj = pb[j];
        for (int b = 0; b < nb; ++b) {
          T v = px[b * f.sx + j];
          if (pa) v *= PI ? pa[b * f.sa + j] : a;
          v += (PI ? pb[b * f.sb + j] : bj) * pc[b * f.sc + ix];
          u[b * P + j] = v;
        }
      }
      continue;
    }
#pragma unroll
    for (int g0 = 0; g0 < NIMG; g0 += G) {
      unsigned jj[G];
      bool ok[G];
      constexpr int NA = PI ? NBM : 1;  // A / xi0 values per image
      T av[G][NA], bv[G][NA], xv[G][NBM], rv[G][NBM];
#pragma unroll
      for (int i = 0; i < G; ++i) {
        ok[i] = image(g0 + i, jj[i]);
        const unsigned j = jj[i];
#pragma unroll
        for (int b = 0; b < NA; ++b) {
          av[i][b] = (T)1;
          bv[i][b] = (T)0;
        }
#pragma unroll
        for (int b = 0; b < NBM; ++b) xv[i][b] = rv[i][b] = (T)0;
        if (!ok[i]) continue;
#pragma unroll
        for (int b = 0; b < NA; ++b) {
          if (b >= nb) break;
          if (pa) av[i][b] = pa[b * f.sa + j];
          bv[i][b] = pb[b * f.sb + j];
        }
#pragma unroll
        for (int b = 0; b < NBM; ++b) {
          if (b >= nb) break;
          xv[i][b] = px[b * f.sx + j];
          if (dirc && live[b]) rv[i][b] = pr[b * f.sx + j];
        }
      }
#pragma unroll
      for (int i = 0; i < G; ++i) {
        if (!ok[i]) continue;
        const unsigned j = jj[i];
#pragma unroll
        for (int b = 0; b < NBM; ++b) {
          if (b >= nb) break;
          T v = xv[i][b];
          if (dirc && live[b]) {
            v = bt[b] * v + rv[i][b];
            pd[b * f.sx + j] = v;
            dd[b] += (double)v * (double)v;
          }
          if (pa) v *= av[i][PI ? b : 0];
          v += bv[i][PI ? b : 0] * cv[b];
          u[b * P + j] = v;
        }
      }
    }
  }
  if (dirc) {
    // per item: wave shuffles, then the four waves in order (fixed order)
    __shared__ double dsh[4][NBM];
#pragma unroll
    for (int b = 0; b < NBM; ++b) {
      double v = dd[b];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if ((threadIdx.x & 63) == 0) dsh[threadIdx.x >> 6][b] = v;
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)nb && threadIdx.x < (unsigned)NBM) {
      const int b = threadIdx.x;
      const double t = ((dsh[0][b] + dsh[1][b]) + dsh[2][b]) + dsh[3][b];
      f.dpart[b * f.dps + f.dblk0 + blockIdx.x] = live[b] ? f.dshift * t : 0.0;
    }
  }
}

// Row-staged folded prologue (D >= 2): one workgroup per group of mirror
// rows -- the 2^(D-1) rows (over the first D-1 axes) that share one row of
// fundamental cells.  The dA runs of that cell row are gathered once into LDS
// (one gather per cell, as pro_fold_kernel), then every row of the group is
// streamed position by position: x, r, A, xi0 loads and d, u stores are
// contiguous, cache-line-aligned runs (pro_fold_kernel's mirrored images
// cross a line boundary in every wave, PMC 1.2x of the algorithmic bytes).
// Same arithmetic per element (bitwise u and d); the d.d partials are per
// row group (nft_hartley_dir_blocks).
// The row's dA runs take (nlast/2 + 1) * NBM * sizeof(T) bytes of dynamic LDS
// beside the kernel's static d.d array (4 * NBM doubles); the bound is the
// worst case (fp64, NBM = 8) of the 160 KB LDS, so that it holds for every
// dtype and batch and nft_hartley_dir_blocks (which knows neither) agrees
// with the launch: 2556 * 64 + 256 <= 163840.
constexpr long long PRO_ROWS_MAXH = (160 * 1024 - 4 * 8 * 8) / (8 * 8);
__host__ __device__ inline bool pro_rows_ok(int D, long long nlast) {
  return D >= 2 && nlast / 2 + 1 <= PRO_ROWS_MAXH;
}
// workgroups (= d.d partial slots) of the row-staged prologue
__host__ __device__ inline long long pro_rows_groups(int D, const long long* n) {
  long long nrg = 1;
  for (int a = 0; a < D - 1; ++a) nrg *= n[a] / 2 + 1;
  return nrg;
}

template <typename T, int D, int NBM, bool PI>
__global__ __launch_bounds__(256) void pro_rows_kernel(fast::FuseArgs f, T* __restrict__ u, long long P, int nb) {
  extern __shared__ __align__(16) unsigned char pro_smem[];
  T* cvs = (T*)pro_smem;  // [hl][NBM]: the dA run of every cell of the row
  const T* __restrict__ px = (const T*)f.px;
  const T* __restrict__ pa = (const T*)f.pa;
  const T* __restrict__ pb = (const T*)f.pb;
  const T* __restrict__ pc = (const T*)f.pc;
  using V2 = typename std::conditional<sizeof(T) == 8, double2, float2>::type;
  const bool vec = f.ce == nb && f.sc == 1 && (nb & 1) == 0 && nb <= NBM;
  const bool dirc = f.dr != nullptr;
  T* pd = const_cast<T*>(px);
  const T* __restrict__ pr = (const T*)f.dr;
  // deferred iterate: item b's previous direction in ring slot s (0: px), the
  // new one into slot s + 1
  const bool lazy = dirc && f.lazy;
  const T* pxs[NBM];
  T* pds[NBM];
#pragma unroll
  for (int b = 0; b < NBM; ++b) {
    pxs[b] = px;
    pds[b] = pd;
    if (lazy && b < nb) {
      // (clamped: a counter out of range never addresses outside the ring)
      const long long sl = min(max((long long)f.dsc[b * NFT_CG_NSCALARS + NFT_CG_LAZY], 0LL), f.lnslot - 1);
      pxs[b] = sl == 0 ? px : (const T*)f.lring + (sl - 1) * f.lss;
      pds[b] = (T*)f.lring + sl * f.lss;
    }
  }
  T bt[NBM];
  bool live[NBM];
  double dd[NBM];
#pragma unroll
  for (int b = 0; b < NBM; ++b) {
    dd[b] = 0.0;
    bt[b] = (T)0;
    live[b] = false;
    if (dirc && b < nb) {
      const double* scb = f.dsc + b * NFT_CG_NSCALARS;
      live[b] = scb[NFT_CG_DONE] == 0.0;
      double beta = scb[NFT_CG_GAMMA] / scb[NFT_CG_GPREV];
      if (!(beta > 0.0)) beta = 0.0;
      bt[b] = (T)beta;
    }
  }
  unsigned nn[D];
#pragma unroll
  for (int a = 0; a < D; ++a) nn[a] = (unsigned)f.fn[a];
  const unsigned n = nn[D - 1], hl = n / 2 + 1;
  unsigned cc[D];
  {
    unsigned rest = blockIdx.x;
#pragma unroll
    for (int a = D - 2; a >= 0; --a) {
      const unsigned h = nn[a] / 2 + 1;
      const unsigned q = rest / h;
      cc[a] = rest - q * h;
      rest = q;
    }
  }
  unsigned cell0 = 0;
#pragma unroll
  for (int a = 0; a < D - 1; ++a) cell0 = cell0 * (nn[a] / 2 + 1) + cc[a];
  cell0 *= hl;
  const int tid = threadIdx.x;
  for (unsigned c1 = tid; c1 < hl; c1 += 256) {
    const long long ix = (long long)f.pidx[cell0 + c1] * f.ce;
    T cv[NBM];
#pragma unroll
    for (int b = 0; b < NBM; ++b) cv[b] = (T)0;
    if (vec) {
      const V2* q = (const V2*)(pc + ix);
#pragma unroll
      for (int bp = 0; bp < NBM / 2; ++bp)
        if (2 * bp < nb) {
          const V2 c2 = q[bp];
          cv[2 * bp] = c2.x;
          cv[2 * bp + 1] = c2.y;
        }
    } else {
#pragma unroll
      for (int b = 0; b < NBM; ++b)
        if (b < nb) cv[b] = pc[b * f.sc + ix];
    }
#pragma unroll
    for (int b = 0; b < NBM; ++b) cvs[c1 * NBM + b] = cv[b];
  }
  __syncthreads();
  constexpr int NROW = 1 << (D - 1);
  constexpr int NA = PI ? NBM : 1;
  constexpr int PRO_RG = NBM <= 2 ? 4 : (NBM == 4 ? 2 : 1);  // positions per thread per load group
#pragma unroll 1
  for (int m = 0; m < NROW; ++m) {
    // row m of the group: bit a of m flips axis a (skipped when self-mirror)
    unsigned rb = 0;
    bool dup = false;
#pragma unroll
    for (int a = 0; a < D - 1; ++a) {
      unsigned k = cc[a];
      if ((m >> a) & 1) {
        const unsigned km = k == 0 ? 0 : nn[a] - k;
        if (km == k) dup = true;
        k = km;
      }
      rb = rb * nn[a] + k;
    }
    if (dup) continue;
    rb *= n;
#pragma unroll 1
    for (unsigned p0 = 0; p0 < n; p0 += 256 * PRO_RG) {
      // every load of the group before its first store (d is stored back
      // into the array x is read from)
      T av[PRO_RG][NA], bv[PRO_RG][NA], xv[PRO_RG][NBM], rv[PRO_RG][NBM];
      bool ok[PRO_RG];
#pragma unroll
      for (int i = 0; i < PRO_RG; ++i) {
        const unsigned pos = p0 + i * 256 + tid;
        ok[i] = pos < n;
        const unsigned j = rb + pos;
#pragma unroll
        for (int b = 0; b < NA; ++b) {
          av[i][b] = (T)1;
          bv[i][b] = (T)0;
          if (ok[i] && b < nb) {
            if (pa) av[i][b] = pa[b * f.sa + j];
            bv[i][b] = pb[b * f.sb + j];
          }
        }
#pragma unroll
        for (int b = 0; b < NBM; ++b) {
          xv[i][b] = rv[i][b] = (T)0;
          if (ok[i] && b < nb) {
            xv[i][b] = pxs[b][b * f.sx + j];
            if (dirc && live[b]) rv[i][b] = pr[b * f.sx + j];
          }
        }
      }
#pragma unroll
      for (int i = 0; i < PRO_RG; ++i) {
        if (!ok[i]) continue;
        const unsigned pos = p0 + i * 256 + tid;
        const unsigned j = rb + pos;
        const unsigned c1 = pos == 0 ? 0 : (pos <= n - pos ? pos : n - pos);
#pragma unroll
        for (int b = 0; b < NBM; ++b) {
          if (b >= nb) break;
          T v = xv[i][b];
          if (dirc && live[b]) {
            v = bt[b] * v + rv[i][b];
            pds[b][b * f.sx + j] = v;
            dd[b] += (double)v * (double)v;
          } else if (lazy) {
            pds[b][b * f.sx + j] = v;  // a stopped item's direction carried to the next slot
          }
          if (pa) v *= av[i][PI ? b : 0];
          v += bv[i][PI ? b : 0] * cvs[c1 * NBM + b];
          u[b * P + j] = v;
        }
      }
    }
  }
  if (dirc) {
    __shared__ double dsh[4][NBM];
#pragma unroll
    for (int b = 0; b < NBM; ++b) {
      double v = dd[b];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if ((threadIdx.x & 63) == 0) dsh[threadIdx.x >> 6][b] = v;
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)nb && threadIdx.x < (unsigned)NBM) {
      const int b = threadIdx.x;
      const double t = ((dsh[0][b] + dsh[1][b]) + dsh[2][b]) + dsh[3][b];
      f.dpart[b * f.dps + f.dblk0 + blockIdx.x] = live[b] ? f.dshift * t : 0.0;
    }
  }
}

template <typename T, int D, int NBM, bool PI>
static int launch_pro_rows_n(const fast::FuseArgs& f, T* u, hipStream_t s) {
  const long long nrg = pro_rows_groups(D, f.fn);
  const size_t lds = (size_t)(f.fn[D - 1] / 2 + 1) * NBM * sizeof(T);
  if (lds > 65536) {
    // the attribute of this instance raised to the largest size asked so far
    // (a later call on a longer last axis needs more than an earlier one)
    static size_t set = 0;
    if (lds > set) {
      NFT_HIP_CHECK(hipFuncSetAttribute((const void*)pro_rows_kernel<T, D, NBM, PI>,
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      set = lds;
    }
  }
  hipLaunchKernelGGL((pro_rows_kernel<T, D, NBM, PI>), dim3((unsigned)nrg), dim3(256), lds, s, f, u, f.P, f.nb);
  return NFT_OK;
}

template <typename T, int D, bool PI>
static int launch_pro_rows(const fast::FuseArgs& f, T* u, hipStream_t s) {
  if (f.nb <= 2) return launch_pro_rows_n<T, D, 2, PI>(f, u, s);
  if (f.nb <= 4) return launch_pro_rows_n<T, D, 4, PI>(f, u, s);
  return launch_pro_rows_n<T, D, 8, PI>(f, u, s);
}

template <typename T, int D, bool PI>
static void launch_pro_fold_pi(const fast::FuseArgs& f, T* u, long long ncell, hipStream_t s) {
  const dim3 grid((unsigned)((ncell + 255) / 256));
  if (f.nb <= 2)
    hipLaunchKernelGGL((pro_fold_kernel<T, D, 2, PI>), grid, dim3(256), 0, s, f, u, f.P, f.nb, ncell);
  else if (f.nb <= 4)
    hipLaunchKernelGGL((pro_fold_kernel<T, D, 4, PI>), grid, dim3(256), 0, s, f, u, f.P, f.nb, ncell);
  else
    hipLaunchKernelGGL((pro_fold_kernel<T, D, 8, PI>), grid, dim3(256), 0, s, f, u, f.P, f.nb, ncell);
}

template <typename T, int D>
static void launch_pro_fold(const fast::FuseArgs& f, T* u, long long ncell, hipStream_t s) {
  if (f.sa != 0 || f.sb != 0)
    launch_pro_fold_pi<T, D, true>(f, u, ncell, s);
  else
    launch_pro_fold_pi<T, D, false>(f, u, ncell, s);
}

// the fused prologue + R2C pass of nft_pro_r2c.hip (done: it ran and wrote
// the half spectra to ws)
int pro_r2c_try(const fast::FuseArgs& f, int dtype, int nd, const long long* shape, int naxes, const int* ax,
                void* ws, size_t hws, hipStream_t s, bool* done);

template <typename T>
static int hartley_fused_impl(const fast::FuseArgs& f, const void* in, void* out, const Geo& g,
                              const std::vector<int>& ax, int sigma, double scale, void* ws, size_t ws_bytes,
                              size_t hws, hipStream_t s) {
  if (f.fnrhs > 0 && (f.pro || !v2_multi_ok(g, ax))) {
    // the carried curvature fold needs the plain R2C row pass of engine v2:
    // otherwise it runs as its own launch first (the same sums)
    int st = nft_fold_partials(f.fpart, f.fnb, f.fnrhs, f.fout, f.fos, s);
    if (st != NFT_OK) return st;
    fast::FuseArgs f1 = f;
    f1.fnrhs = 0;
    return hartley_fused_impl<T>(f1, in, out, g, ax, sigma, scale, ws, ws_bytes, hws, s);
  }
  const long long ntot = prod(g.shape, 0, g.nd);
  if (f.dr && !(f.fnd > 0 && f.pb && f.sa == 0 && f.sb == 0 && f.P > 0 &&
                (long long)f.nb * f.P == ntot && ws_bytes >= align256(hws) + (size_t)ntot * sizeof(T))) {
    set_last_error("nft_hartley_fused: the direction carried by the prologue needs the folded batched prologue pass");
    return NFT_ERR_UNSUPPORTED;
  }
  // a single folded item (P = 0) takes the split path too, as a batch of one:
  // the in-pass prologue measured 116 us at 2048^2 against about 45 for the
  // folded pass + the plain persistent R2C pass.  Per-item A / xi0 take the
  // folded prologue pass as well (not the in-pass prologue of the R2C pass).
  if (!f.dr && f.P == 0 && f.fnd > 0 && f.pb && f.pro && ws_bytes >= align256(hws) + (size_t)ntot * sizeof(T)) {
    fast::FuseArgs f1 = f;
    f1.P = ntot;
    f1.nb = 1;
    f1.pshift = -1;
    if ((ntot & (ntot - 1)) == 0) {
      int sh = 0;
      while ((1LL << sh) < ntot) ++sh;
      f1.pshift = sh;
    }
    f1.sx = f1.so = f1.sd = f1.s2 = ntot;
    return hartley_fused_impl<T>(f1, in, out, g, ax, sigma, scale, ws, ws_bytes, hws, s);
  }
  // per-item A / xi0 (f.sa, f.sb != 0) take the folded pass too (no carried direction)
  const bool shared_ab = f.sa == 0 && f.sb == 0;
  if (f.pro && (f.pa || f.pb) && (shared_ab || (f.fnd > 0 && f.pb && !f.dr)) &&
      f.P > 0 && (f.nb > 1 || f.dr || f.fnd > 0) &&
      (long long)f.nb * f.P == ntot &&
      ws_bytes >= align256(hws) + (size_t)ntot * sizeof(T)) {
    T* u = (T*)((char*)ws + align256(hws));
    // one element per thread (no grid-stride chain of dependent gathers)
    const unsigned nblk = (unsigned)((f.P + 255) / 256);
    {
      bool done = false;
      int pst = pro_r2c_try(f, sizeof(T) == 8 ? 0 : 1, g.nd, g.shape, (int)ax.size(), ax.data(), ws, hws, s, &done);
      if (pst != NFT_OK) return pst;
      if (done) {
        fast::FuseArgs f2 = f;
        f2.pro = 0;
        f2.px = f2.pa = f2.pb = f2.pc = nullptr;
        f2.pidx = nullptr;
        f2.dr = nullptr;
        return hartley_v2<T>(nullptr, out, g, ax, sigma, scale, ws, hws, s, &f2, true);
      }
    }
    if (f.fnd > 0 && f.pb) {
      long long ncell = 1;  // padded cell grid (pro_fold_kernel)
      for (int a = 0; a < f.fnd; ++a) ncell *= a == f.fnd - 1 ? ((f.fn[a] / 2 + 1 + 63) & ~63LL) : f.fn[a] / 2 + 1;
      prof_mark(s, f.dr ? "pro_fold+dir" : "pro_fold");
      const bool rows = pro_rows_ok(f.fnd, f.fn[f.fnd - 1]) && f.nb <= 8;
      const bool pi = f.sa != 0 || f.sb != 0;
      if (f.lazy && f.dr && !(rows && f.fnd >= 2)) {
        set_last_error("nft_hartley_fused: the deferred iterate needs the row-staged prologue");
        return NFT_ERR_UNSUPPORTED;
      }
      int pst = NFT_OK;
      if (rows && f.fnd == 2)
        pst = pi ? launch_pro_rows<T, 2, true>(f, u, s) : launch_pro_rows<T, 2, false>(f, u, s);
      else if (rows && f.fnd == 3)
        pst = pi ? launch_pro_rows<T, 3, true>(f, u, s) : launch_pro_rows<T, 3, false>(f, u, s);
      else if (f.fnd == 1)
        launch_pro_fold<T, 1>(f, u, ncell, s);
      else if (f.fnd == 2)
        launch_pro_fold<T, 2>(f, u, ncell, s);
      else
        launch_pro_fold<T, 3>(f, u, ncell, s);
      if (pst != NFT_OK) return pst;
    } else {
      prof_mark(s, "pro_batch");
      hipLaunchKernelGGL(pro_batch_kernel<T>, dim3(nblk), dim3(256), 0, s, f, u, f.P, f.nb);
    }
    NFT_HIP_CHECK(hipGetLastError());
    fast::FuseArgs f2 = f;
    f2.pro = 0;
    f2.px = f2.pa = f2.pb = f2.pc = nullptr;
    f2.pidx = nullptr;
    int st = hartley_v2<T>(u, out, g, ax, sigma, scale, ws, hws, s, &f2);
    if (st != NFT_FALLBACK) return st;
    return hartley_fused_impl<T>(f2, u, out, g, ax, sigma, scale, ws, ws_bytes, hws, s);
  }
  {
    int st = hartley_v2<T>(in, out, g, ax, sigma, scale, ws, ws_bytes, s, &f);
    if (st != NFT_FALLBACK) return st;
  }
  if (f.cg || f.o2h || f.quad) {
    set_last_error("nft_hartley_fused: the CG-carrying / quadratic-form epilogue / out2 pair sums need the "
                   "engine-v2 unpack pass "
                   "(nft_hartley_cg_blocks == 0 for this geometry)");
    return NFT_ERR_UNSUPPORTED;
  }
  const long long n = prod(g.shape, 0, g.nd);
  const unsigned nb = (unsigned)std::min<long long>((n + 255) / 256, 65536);
  const void* src = in;
  if (f.pro) {
    if (ws_bytes < align256(hws) + (size_t)n * sizeof(T)) {
      set_last_error("hartley_fused workspace too small");
      return NFT_ERR_ARG;
    }
    T* tmp = (T*)((char*)ws + align256(hws));
    hipLaunchKernelGGL(fuse_pro_kernel<T>, dim3(nb), dim3(256), 0, s, f, tmp, n);
    NFT_HIP_CHECK(hipGetLastError());
    src = tmp;
  }
  // with an epilogue the transform goes to a second temporary: the epilogue's
  // output may use a different batch layout than the transform's
  T* dst = (T*)out;
  if (f.epi) {
    if (ws_bytes < align256(hws) + 2 * (size_t)n * sizeof(T)) {
      set_last_error("hartley_fused workspace too small");
      return NFT_ERR_ARG;
    }
    dst = (T*)((char*)ws + align256(hws)) + n;
  }
  int st = hartley_impl<T>(src, dst, g, ax, sigma, scale, ws, hws, s);
  if (st != NFT_OK) return st;
  if (f.epi) {
    hipLaunchKernelGGL(fuse_epi_kernel<T>, dim3(nb), dim3(256), 0, s, f, (const T*)dst, (T*)out, n);
    NFT_HIP_CHECK(hipGetLastError());
  }
  return NFT_OK;
}

template <typename T>
static int c2c_impl(const void* in, void* out, const Geo& g, const std::vector<int>& ax, int forward,
                    double scale, hipStream_t s) {
  const int m = (int)ax.size();
  if (m == 0) {
    long long N = prod(g.shape, 0, g.nd);
    if (in != out)
      NFT_HIP_CHECK(hipMemcpyAsync(out, in, N * sizeof(cplx_t<T>), hipMemcpyDeviceToDevice, s));
    if (scale != 1.0) return scale_real(out, 2 * N, sizeof(T) == 8 ? 0 : 1, scale, s);
    return NFT_OK;
  }
  for (int k = m - 1; k >= 0; --k) {
    int axis = ax[k];
    PassArgs<T> a;
    memset(&a, 0, sizeof(a));
    a.plan = make_plan((int)g.shape[axis]);
    a.in = (k == m - 1) ? in : out;
    a.out = out;
    fill_line_geom(a, g.shape, g.shape, g.nd, axis);
    a.conj_in = forward ? 0 : 1;
    a.conj_out = forward ? 0 : 1;
    a.scale = (T)(k == 0 ? scale : 1.0);
    int st = launch_pass<T>(PK_C2C, a, s);
    if (st != NFT_OK) return st;
  }
  return NFT_OK;
}

// one engine-v2 fp64 pass for the other translation units (nft_conv.hip)
int fast_pass_f64(int kind, bool rows, int N, fast::FastArgs<double>& a, hipStream_t s) {
  return fast::launch<double>(kind, rows, N, a, s);
}

}  // namespace nft

using namespace nft;

extern "C" {

const char* nft_last_error(void) { return nft::last_error(); }

int nft_hartley_workspace(int ndim, const int64_t* shape, int naxes, const int* axes, int dtype,
                          size_t* bytes) {
  Geo g;
  std::vector<int> ax;
  int st = parse_axes(ndim, shape, naxes, axes, g, ax);
  if (st != NFT_OK) return st;
  if (ax.size() < 2) {
    *bytes = 0;
    return NFT_OK;
  }
  long long cs[MAXD];
  half_shape(g, ax.back(), cs);
  size_t es = dtype == 0 ? sizeof(double2) : sizeof(float2);
  *bytes = (size_t)prod(cs, 0, g.nd) * es;
  return NFT_OK;
}

int nft_hartley(const void* in, void* out, int ndim, const int64_t* shape, int naxes,
                const int* axes, int dtype, int convention, double scale, void* workspace,
                size_t ws_bytes, hipStream_t stream) {
  Geo g;
  std::vector<int> ax;
  int st = parse_axes(ndim, shape, naxes, axes, g, ax);
  if (st != NFT_OK) return st;
  int sigma = convention == 0 ? 1 : -1;
  if (dtype == 0 || dtype == 1) {
    if (dtype == 0) st = hartley_v2<double>(in, out, g, ax, sigma, scale, workspace, ws_bytes, stream);
    else if (dtype == 1) st = hartley_v2<float>(in, out, g, ax, sigma, scale, workspace, ws_bytes, stream);
    if (st != NFT_FALLBACK) return st;
  }
  if (dtype == 0) return hartley_impl<double>(in, out, g, ax, sigma, scale, workspace, ws_bytes, stream);
  if (dtype == 1) return hartley_impl<float>(in, out, g, ax, sigma, scale, workspace, ws_bytes, stream);
  set_last_error("bad dtype %d", dtype);
  return NFT_ERR_ARG;
}

int nft_hartley_fused_workspace(int ndim, const int64_t* shape, int naxes, const int* axes, int dtype,
                                size_t* bytes) {
  int st = nft_hartley_workspace(ndim, shape, naxes, axes, dtype, bytes);
  if (st != NFT_OK) return st;
  long long n = 1;
  for (int d = 0; d < ndim; ++d) n *= shape[d];
  *bytes = align256(*bytes) + 2 * (size_t)n * (dtype == 0 ? 8 : 4);
  return NFT_OK;
}

int nft_hartley_fused(const nft_hartley_fuse* fz, const void* in, void* out, int ndim, const int64_t* shape,
                      int naxes, const int* axes, int dtype, int convention, double scale, void* workspace,
                      size_t ws_bytes, hipStream_t stream) {
  Geo g;
  std::vector<int> ax;
  int st = parse_axes(ndim, shape, naxes, axes, g, ax);
  if (st != NFT_OK) return st;
  size_t hws = 0;
  if ((st = nft_hartley_workspace(ndim, shape, naxes, axes, dtype, &hws)) != NFT_OK) return st;
  fast::FuseArgs f;
  memset(&f, 0, sizeof(f));
  if (fz) {
    f.pa = fz->pro_a;
    f.px = fz->pro_x;
    f.pb = fz->pro_b;
    f.pc = fz->pro_c;
    f.pidx = fz->pro_index;
    f.ea = fz->epi_a;
    f.ed = fz->epi_d;
    f.eb = fz->epi_b;
    f.out2 = fz->epi_out2;
    f.eshift = fz->epi_shift;
    f.pro = f.px != nullptr;
    f.epi = (f.ea || f.ed || f.out2) ? 1 : 0;
    f.P = fz->batch_period;
    f.nb = 0;
    if (f.P > 0) {
      long long tot = 1;
      for (int d = 0; d < ndim; ++d) tot *= shape[d];
      f.nb = (int)(tot / f.P);
    }
    f.pshift = -1;
    if (f.P > 0 && (f.P & (f.P - 1)) == 0) {
      int sh = 0;
      while ((1LL << sh) < f.P) ++sh;
      f.pshift = sh;
    }
    f.sx = fz->x_bstride ? fz->x_bstride : f.P;
    f.sc = fz->c_bstride;
    f.ce = fz->c_estride > 0 ? fz->c_estride : 1;
    f.sa = fz->a_bstride;
    f.sb = fz->b_bstride;
    f.sea = fz->ea_bstride;
    f.seb = fz->eb_bstride;
    if (f.P == 0) f.sa = f.sb = f.sea = f.seb = 0;
    f.so = fz->out_bstride ? fz->out_bstride : f.P;
    f.sd = fz->d_bstride ? fz->d_bstride : f.P;
    f.s2 = fz->out2_bstride ? fz->out2_bstride : f.P;
    if (f.P < 0 || (f.P > 0 && f.pb && f.sc == 0)) {
      set_last_error("nft_hartley_fused: batch needs c_bstride");
      return NFT_ERR_ARG;
    }
    f.fnd = 0;
    if (fz->pro_folded && f.pb) {
      // item grid = the transform axes (in order); fold strides over n/2+1
      long long per = 1;
      for (int a : ax) per *= shape[a];
      if ((int)ax.size() > 3 || per != (f.P > 0 ? f.P : per) ||
          (f.P > 0 && ax.size() + 1 != (size_t)ndim) || (f.P == 0 && ax.size() != (size_t)ndim)) {
        set_last_error("nft_hartley_fused: pro_folded needs the transform axes to span each item");
        return NFT_ERR_ARG;
      }
      f.fnd = (int)ax.size();
      long long st = 1;
      for (int a = f.fnd - 1; a >= 0; --a) {
        f.fn[a] = shape[ax[a]];
        f.fs[a] = st;
        st *= shape[ax[a]] / 2 + 1;
      }
    }
    if ((f.pb && (!f.pc || !f.pidx)) || (f.out2 && !f.eb)) {
      set_last_error("nft_hartley_fused: incomplete fusion spec");
      return NFT_ERR_ARG;
    }
    f.o2h = 0;
    if (fz->epi_out2_pairs) {
      if (!f.out2 || !f.eb || ax.empty() || ax.back() != ndim - 1) {
        set_last_error("nft_hartley_fused: epi_out2_pairs needs out2, epi_b and the last axis transformed");
        return NFT_ERR_ARG;
      }
      f.o2h = 1;
      f.nlast = shape[ndim - 1];
      f.nh = shape[ndim - 1] / 2 + 1;
    }
    f.dr = nullptr;
    if (fz->dir_r) {
      if (!fz->pro_folded || !f.pb || f.P <= 0 || f.nb < 1 || f.nb > 8 || !fz->dir_sc || !fz->dir_part ||
          fz->dir_blk0 < 0 || fz->dir_pstride < fz->dir_blk0 + nft_hartley_dir_blocks(f.fnd, (const int64_t*)f.fn)) {
        set_last_error("nft_hartley_fused: the direction carried by the prologue needs a folded, batched "
                       "prologue (<= 8 items) and its scalars / partials");
        return NFT_ERR_ARG;
      }
      f.dr = fz->dir_r;
      f.dsc = fz->dir_sc;
      f.dpart = fz->dir_part;
      f.dps = fz->dir_pstride;
      f.dshift = fz->dir_shift;
      f.dblk0 = fz->dir_blk0;
    }
    f.cg = 0;
    if (fz->cg_x) {
      if (!fz->cg_r || !fz->cg_d || !fz->cg_sc || !fz->cg_part || fz->cg_nbtot < 1 || fz->cg_blk0 < 0 ||
          f.P <= 0 || f.ed || !f.epi ||
          nft_hartley_cg_blocks(ndim, shape, naxes, axes, dtype) + fz->cg_blk0 > fz->cg_nbtot) {
        set_last_error("nft_hartley_fused: incomplete or unsupported CG epilogue spec");
        return NFT_ERR_ARG;
      }
      f.cg = 1;
      f.cx = fz->cg_x;
      f.cr = fz->cg_r;
      f.cd = fz->cg_d;
      f.csc = fz->cg_sc;
      f.cpart = fz->cg_part;
      f.cst = fz->cg_stride;
      f.cshift = fz->cg_shift;
      f.cnbtot = fz->cg_nbtot;
      f.cblk0 = fz->cg_blk0;
    }
    f.quad = 0;
    if (fz->quad_part) {
      if (f.cg || !f.ea || f.ed || f.out2 || f.P <= 0 || f.nb < 1 || fz->quad_blk0 < 0 ||
          fz->quad_pstride < fz->quad_blk0 + nft_hartley_cg_blocks(ndim, shape, naxes, axes, dtype)) {
        set_last_error("nft_hartley_fused: the quadratic-form epilogue needs a batch, epi_a alone and "
                       "quad_pstride >= quad_blk0 + nft_hartley_cg_blocks");
        return NFT_ERR_ARG;
      }
      f.quad = 1;
      f.qpart = fz->quad_part;
      f.qps = fz->quad_pstride;
      f.qblk0 = fz->quad_blk0;
    }
    f.lazy = 0;
    if (fz->lazy_ring) {
      if (!fz->lazy_alpha || fz->lazy_nslot < 1 || fz->lazy_sstride < 1 || !(f.dr || f.cg)) {
        set_last_error("nft_hartley_fused: the deferred iterate needs its alphas, slots and the carried "
                       "direction or CG epilogue");
        return NFT_ERR_ARG;
      }
      f.lazy = 1;
      f.lring = fz->lazy_ring;
      f.lss = fz->lazy_sstride;
      f.lalpha = fz->lazy_alpha;
      f.lnslot = fz->lazy_nslot;
    }
    f.fnrhs = 0;
    if (fz->fold_nrhs > 0) {
      if (!fz->fold_part || !fz->fold_out || fz->fold_nb < 1 || fz->fold_nb > 0x7fffffffLL ||
          fz->fold_nrhs > 65535 || fz->fold_ostride < 1) {
        set_last_error("nft_hartley_fused: the carried fold needs its partials, output, 1 <= fold_nb, "
                       "fold_nrhs <= 65535 and fold_ostride >= 1");
        return NFT_ERR_ARG;
      }
      f.fpart = fz->fold_part;
      f.fout = fz->fold_out;
      f.fos = fz->fold_ostride;
      f.fnb = (int)fz->fold_nb;
      f.fnrhs = (int)fz->fold_nrhs;
    }
  }
  const int sigma = convention == 0 ? 1 : -1;
  if (dtype == 0) return hartley_fused_impl<double>(f, in, out, g, ax, sigma, scale, workspace, ws_bytes, hws, stream);
  if (dtype == 1) return hartley_fused_impl<float>(f, in, out, g, ax, sigma, scale, workspace, ws_bytes, hws, stream);
  set_last_error("bad dtype %d", dtype);
  return NFT_ERR_ARG;
}

int nft_hartley_dir_blocks(int ndim, const int64_t* shape) {
  if (ndim < 1 || ndim > 3 || !shape) return 0;
  for (int a = 0; a < ndim; ++a)
    if (shape[a] < 1) return 0;
  if (pro_rows_ok(ndim, shape[ndim - 1])) {
    // the row-staged prologue: one block per group of mirror rows
    long long n[3];
    for (int a = 0; a < ndim; ++a) n[a] = shape[a];
    return (int)pro_rows_groups(ndim, n);
  }
  long long ncell = 1;
  for (int a = 0; a < ndim; ++a) {
    if (shape[a] < 1) return 0;
    ncell *= a == ndim - 1 ? ((shape[a] / 2 + 1 + 63) & ~63LL) : shape[a] / 2 + 1;
  }
  return (int)((ncell + 255) / 256);
}

int nft_hartley_pro_rows(int ndim, const int64_t* shape) {
  if (ndim < 1 || ndim > 3 || !shape) return 0;
  for (int a = 0; a < ndim; ++a)
    if (shape[a] < 1) return 0;
  return pro_rows_ok(ndim, shape[ndim - 1]) ? 1 : 0;
}

int nft_hartley_cg_blocks(int ndim, const int64_t* shape, int naxes, const int* axes, int dtype) {
  using namespace fast;
  Geo g;
  std::vector<int> ax;
  if (parse_axes(ndim, shape, naxes, axes, g, ax) != NFT_OK) return 0;
  const int m = (int)ax.size();
  const int last = g.nd - 1;
  // a leading batch axis and the engine-v2 strided last pass along ax[0] = 1
  if (m < 2 || g.nd != m + 1 || ax[0] != 1 || (dtype != 0 && dtype != 1)) return 0;
  const int h = ax[m - 1];
  if (h != last || !rows_supported((int)g.shape[h])) return 0;
  for (int k = 1; k < m - 1; ++k)
    if (!strided_supported((int)g.shape[ax[k]])) return 0;
  const int N0 = (int)g.shape[ax[0]];
  long long cs[MAXD];
  half_shape(g, h, cs);
  const long long I = prod(cs, ax[0] + 1, g.nd);
  long long M = 1;
  int N = N0;
  if (!strided_supported(N0)) {
    if (!fourstep_supported(N0)) return 0;
    int N1, N2;
    fourstep_split(N0, N1, N2);
    M = N1;
    N = N2;
  }
  const int NT = nt_strided(N);
  const long long L = (long long)NT * fast::VPT / N;
  if (L < 1) return 0;
  const long long tiles = M * ((I + L - 1) / L);
  return tiles > 0x3fffffffLL ? 0 : (int)tiles;
}

int nft_fft_c2c(const void* in, void* out, int ndim, const int64_t* shape, int naxes, const int* axes,
                int dtype, int forward, double scale, hipStream_t stream) {
  Geo g;
  std::vector<int> ax;
  int st = parse_axes(ndim, shape, naxes, axes, g, ax);
  if (st != NFT_OK) return st;
  if (dtype == 0) return c2c_impl<double>(in, out, g, ax, forward, scale, stream);
  if (dtype == 1) return c2c_impl<float>(in, out, g, ax, forward, scale, stream);
  set_last_error("bad dtype %d", dtype);
  return NFT_ERR_ARG;
}

int nft_fft_prepare(int n, int dtype) {
  const void* tw;
  return get_twiddles(n, dtype, &tw);
}

void nft_release_caches(void) { free_twiddles(); }

}  // extern "C"
