// Host-side checks of the nft_matern_* entry points under AddressSanitizer
// (the pattern of abi_host_driver.cpp): sizing arithmetic and the argument
// validation that rejects a call before any launch.  The host code is built
// with -fsanitize=address; no call here reaches the device.  Exit code 0 =
// every check held and ASan reported nothing.
#include <cstdio>
#include <cstring>

#include "nifty_amd.h"

static int fails = 0;
#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                            \
    }                                                                     \
  } while (0)

static bool err_mentions(const char* s) {
  const char* e = nft_last_error();
  return e && std::strstr(e, s) != nullptr;
}

int main() {
  // sizing: three columns padded to an even length; three partials per
  // 512-bin workgroup, padded to an even count
  CHECK(nft_matern_forward_buf(1) == 0 && nft_matern_workspace(1) == 0);
  CHECK(nft_matern_forward_buf(2) == 6 && nft_matern_forward_buf(29) == 90);
  CHECK(nft_matern_forward_buf(313847) == 3 * 313848);
  CHECK(nft_matern_workspace(2) == 4 * sizeof(double));
  CHECK(nft_matern_workspace(512) == 4 * sizeof(double));
  CHECK(nft_matern_workspace(513) == 6 * sizeof(double));
  CHECK(nft_matern_workspace(313847) == 1840 * sizeof(double));  // 613 workgroups

  double dummy[8] = {0};
  nft_matern_const dc[2];
  // forward
  {
    nft_matern_model m;
    std::memset(&m, 0, sizeof(m));
    m.B = 100;
    m.k2 = dummy;
    m.has_zm = 1;
    CHECK(nft_matern_forward_batched(&m, dummy, dummy, dummy, nullptr, 0, 1, dummy, 100, dummy, 300, dc, nullptr) ==
          NFT_ERR_ARG);  // zero mode without its key
    m.has_zm = 0;
    CHECK(nft_matern_forward_batched(&m, dummy, dummy, dummy, nullptr, 0, 1, dummy, 100, dummy, 299, dc, nullptr) ==
          NFT_ERR_ARG);  // buffer stride too small
    CHECK(nft_matern_forward_batched(&m, dummy, dummy, dummy, nullptr, 0, 2, dummy, 99, dummy, 300, dc, nullptr) ==
          NFT_ERR_ARG);  // rows of a overlap
    CHECK(nft_matern_forward_batched(&m, dummy, dummy, dummy, nullptr, 0, 0, dummy, 100, dummy, 300, dc, nullptr) ==
          NFT_ERR_ARG);  // nrow 0
    CHECK(nft_matern_forward_batched(&m, dummy, nullptr, dummy, nullptr, 0, 1, dummy, 100, dummy, 300, dc,
                                     nullptr) == NFT_ERR_ARG);
    CHECK(nft_matern_forward_batched(&m, dummy, dummy, dummy, nullptr, 0, 1, dummy, 100, dummy, 300, nullptr,
                                     nullptr) == NFT_ERR_ARG);
    m.B = 1;
    CHECK(nft_matern_forward_batched(&m, dummy, dummy, dummy, nullptr, 0, 1, dummy, 100, dummy, 300, dc, nullptr) ==
          NFT_ERR_ARG);
    CHECK(nft_matern_forward_batched(nullptr, dummy, dummy, dummy, nullptr, 0, 1, dummy, 100, dummy, 300, dc,
                                     nullptr) == NFT_ERR_ARG);
    CHECK(err_mentions("nft_matern_forward_batched"));
  }
  nft_matern_const c;
  std::memset(&c, 0, sizeof(c));
  c.B = 100;
  c.gs = c.gc = c.gl = dummy;
  c.has_zm = 1;
  // JVP
  {
    const double* t[4] = {dummy, dummy, dummy, dummy};
    const double* t3[4] = {dummy, dummy, dummy, nullptr};
    const double* t1[4] = {dummy, nullptr, dummy, dummy};
    CHECK(nft_matern_jvp_batched(nullptr, nullptr, 0, t, 8, dummy, 100, 1, 4, 0, nullptr) == NFT_ERR_ARG);
    CHECK(err_mentions("nft_matern_jvp_batched"));
    CHECK(nft_matern_jvp_batched(&c, nullptr, 0, t, 8, dummy, 100, 1, 0, 0, nullptr) == NFT_ERR_ARG);   // nrhs 0
    CHECK(nft_matern_jvp_batched(&c, nullptr, 0, nullptr, 8, dummy, 100, 1, 4, 0, nullptr) == NFT_ERR_ARG);
    CHECK(nft_matern_jvp_batched(&c, nullptr, 0, t1, 8, dummy, 100, 1, 4, 0, nullptr) == NFT_ERR_ARG);
    CHECK(nft_matern_jvp_batched(&c, nullptr, 0, t3, 8, dummy, 100, 1, 4, 0, nullptr) == NFT_ERR_ARG);  // zm key
    CHECK(nft_matern_jvp_batched(&c, nullptr, 0, t, 8, nullptr, 100, 1, 4, 0, nullptr) == NFT_ERR_ARG);
    CHECK(nft_matern_jvp_batched(&c, nullptr, 1, t, 8, dummy, 100, 1, 4, 0, nullptr) == NFT_ERR_ARG);   // no items
    CHECK(nft_matern_jvp_batched(&c, nullptr, 2, t, 8, dummy, 100, 1, 4, 0, nullptr) == NFT_ERR_ARG);
    CHECK(nft_matern_jvp_batched(&c, dc, 3, t, 8, dummy, 100, 1, 4, 0, nullptr) == NFT_ERR_ARG);        // mode
    CHECK(nft_matern_jvp_batched(&c, nullptr, 0, t, 8, dummy, 100, 1, 4, 1, nullptr) == NFT_ERR_ARG);   // fp32
    CHECK(nft_matern_jvp_batched(&c, nullptr, 0, t, 8, dummy, 99, 1, 4, 0, nullptr) == NFT_ERR_ARG);    // planar overlap
    CHECK(nft_matern_jvp_batched(&c, nullptr, 0, t, 8, dummy, 1, 3, 4, 0, nullptr) == NFT_ERR_ARG);     // bin-major overlap
    CHECK(nft_matern_jvp_batched(&c, nullptr, 0, t, 8, dummy, 0, 4, 4, 0, nullptr) == NFT_ERR_ARG);     // all RHS on one row
    CHECK(nft_matern_jvp_batched(&c, nullptr, 0, t, 8, dummy, 100, -1, 4, 0, nullptr) == NFT_ERR_ARG);
    CHECK(nft_matern_jvp_batched(&c, nullptr, 0, t, -8, dummy, 100, 1, 4, 0, nullptr) == NFT_ERR_ARG);
    nft_matern_const nocol = c;
    nocol.gc = nullptr;
    CHECK(nft_matern_jvp_batched(&nocol, nullptr, 0, t, 8, dummy, 100, 1, 4, 0, nullptr) == NFT_ERR_ARG);
    nft_matern_const small = c;
    small.B = 1;
    CHECK(nft_matern_jvp_batched(&small, nullptr, 0, t, 8, dummy, 100, 1, 4, 0, nullptr) == NFT_ERR_ARG);
  }
  // VJP
  {
    double* o[4] = {dummy, dummy, dummy, dummy};
    double* o3[4] = {dummy, dummy, dummy, nullptr};
    const double* d1[4] = {dummy, nullptr, dummy, dummy};
    CHECK(nft_matern_vjp_batched(nullptr, nullptr, 0, dummy, 100, o, nullptr, 8, 0.0, dummy, 4, nullptr) ==
          NFT_ERR_ARG);
    CHECK(err_mentions("nft_matern_vjp_batched"));
    CHECK(nft_matern_vjp_batched(&c, nullptr, 0, dummy, 100, o, nullptr, 8, 0.0, dummy, 0, nullptr) == NFT_ERR_ARG);
    CHECK(nft_matern_vjp_batched(&c, nullptr, 0, nullptr, 100, o, nullptr, 8, 0.0, dummy, 4, nullptr) == NFT_ERR_ARG);
    CHECK(nft_matern_vjp_batched(&c, nullptr, 0, dummy, 100, nullptr, nullptr, 8, 0.0, dummy, 4, nullptr) ==
          NFT_ERR_ARG);
    CHECK(nft_matern_vjp_batched(&c, nullptr, 0, dummy, 100, o3, nullptr, 8, 0.0, dummy, 4, nullptr) == NFT_ERR_ARG);
    CHECK(nft_matern_vjp_batched(&c, nullptr, 0, dummy, 100, o, nullptr, 8, 0.0, nullptr, 4, nullptr) == NFT_ERR_ARG);
    CHECK(nft_matern_vjp_batched(&c, nullptr, 0, dummy, 100, o, d1, 8, 0.5, dummy, 4, nullptr) == NFT_ERR_ARG);
    CHECK(nft_matern_vjp_batched(&c, nullptr, 0, dummy, 99, o, nullptr, 8, 0.0, dummy, 4, nullptr) == NFT_ERR_ARG);  // g rows overlap
    CHECK(nft_matern_vjp_batched(&c, nullptr, 0, dummy, 100, o, nullptr, 0, 0.0, dummy, 4, nullptr) == NFT_ERR_ARG); // outputs overlap
    CHECK(nft_matern_vjp_batched(&c, nullptr, 1, dummy, 100, o, nullptr, 8, 0.0, dummy, 4, nullptr) == NFT_ERR_ARG); // no items
  }
  CHECK(std::strlen(nft_last_error()) < 4096);
  if (fails) {
    std::fprintf(stderr, "%d check(s) failed\n", fails);
    return 1;
  }
  std::printf("matern host checks: ok\n");
  return 0;
}
